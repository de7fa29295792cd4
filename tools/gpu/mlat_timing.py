#!/usr/bin/env python3
"""GPU box helper: device time of multilaterate (adsb_multilaterate_of: the copy of the stations, the mlat_solve kernel
and rocPRIM's reduction of the header) for correlated lists that are already in device memory, measured with device
events on the ctx stream, one process, warm.  The events enclose the whole call, the wait for the 8 KiB station copy
included.  Beside it, the CPU mirror's time for the same list on one core.  No threshold: there is nothing else to
compare it with.

  tools/gpu/mlat_timing.py --out profiles/mlat_timing.txt

The lists: --messages emitters 0-150 km around (47.45, 8.56) at 3-12 km, each heard by all of R receivers on rings of
36-60 km, 1 ns ticks; R = 6 solved free (two stages), R = 6 with the messages' altitudes (one stage), R = 32 free
(two receptions per lane).  The first repetition's fixes are compared with the mirror's."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

A_WGS, F_WGS = 6378137.0, 1.0 / 298.257223563


def ecef(np, lat, lon, h):
    e2 = F_WGS * (2.0 - F_WGS)
    phi, lam = np.radians(lat), np.radians(lon)
    n = A_WGS / np.sqrt(1.0 - e2 * np.sin(phi) ** 2)
    return np.stack([(n + h) * np.cos(phi) * np.cos(lam), (n + h) * np.cos(phi) * np.sin(lam),
                     (n * (1.0 - e2) + h) * np.sin(phi)], axis=-1)


def make_list(np, A, n_msgs, n_receivers, seed):
    """(receivers, messages, receptions) of a correlate result, built directly."""
    rng = np.random.default_rng(seed)
    lat0, lon0 = 47.45, 8.56
    east = lambda d: d / (111200.0 * np.cos(np.radians(lat0)))
    az = 2 * np.pi * (np.arange(n_receivers) + rng.uniform(-0.25, 0.25, n_receivers)) / n_receivers
    rad = rng.uniform(36e3, 60e3, n_receivers)
    rcv = np.zeros(n_receivers, dtype=A.MLAT_RECEIVER_DTYPE)
    rcv["latitude"], rcv["longitude"] = lat0 + rad * np.cos(az) / 111200.0, lon0 + east(rad * np.sin(az))
    rcv["height_m"] = rng.uniform(300.0, 1800.0, n_receivers)
    st = ecef(np, rcv["latitude"], rcv["longitude"], rcv["height_m"])
    az, rad = rng.uniform(0, 2 * np.pi, n_msgs), 150e3 * np.sqrt(rng.uniform(0, 1, n_msgs))
    alt_n = np.round((rng.uniform(3000.0, 12000.0, n_msgs) / 0.3048 + 1000.0) / 25.0).astype(np.int64)
    pos = ecef(np, lat0 + rad * np.cos(az) / 111200.0, lon0 + east(rad * np.sin(az)), (alt_n * 25 - 1000) * 0.3048)
    dist = np.sqrt(((pos[:, None, :] - st[None, :, :]) ** 2).sum(axis=2))
    t = np.floor(((np.arange(n_msgs) + 1)[:, None] * 2e-3 + dist / A.ADSB_MLAT_C) / 1e-9).astype(np.uint64)
    order = np.argsort(t, axis=1, kind="stable")
    recs = np.zeros(n_msgs * n_receivers, dtype=A.RECEPTION_DTYPE)
    recs["time"] = np.take_along_axis(t, order, axis=1).reshape(-1)
    recs["receiver"] = order.reshape(-1)
    recs["frame"] = np.arange(len(recs))
    msgs = np.zeros(n_msgs, dtype=A.MESSAGE_DTYPE)
    code = (alt_n >> 4) << 5 | 0x10 | (alt_n & 0xF)
    msgs["bytes"][:, 0], msgs["bytes"][:, 4] = 0x8D, 11 << 3
    msgs["bytes"][:, 5], msgs["bytes"][:, 6] = code >> 4, (code & 0xF) << 4
    msgs["first"] = np.arange(n_msgs) * n_receivers
    msgs["n_receptions"] = msgs["n_receivers"] = n_receivers
    msgs["time"] = recs["time"][::n_receivers]
    return rcv, msgs, recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--messages", type=int, default=32768)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", help="also write the report to this file")
    args = ap.parse_args()

    import numpy as np
    import torch

    import air_rs_amd as A

    torch.cuda.set_stream(torch.cuda.Stream())  # a stream of our own: a NULL stream would make the ctx create one
    stream = torch.cuda.current_stream()
    dem = A.AdsbDemod(device=0, max_samples=1 << 16, max_out=1024, stream=stream.cuda_stream, host_staging=False)

    def timed(call):
        """median, min, max in us of `call` alone between two events, the stream idle before the first"""
        ms = []
        for _ in range(args.warmup + args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record(stream)
            call()
            b.record(stream)
            b.synchronize()
            ms.append(a.elapsed_time(b))
        us = np.array(ms[args.warmup:]) * 1e3
        return float(np.median(us)), float(us.min()), float(us.max())

    lines = []
    n = args.messages
    for name, R, alt in (("6 receivers, free", 6, False), ("6 receivers, altitude", 6, True), ("32 receivers, free", 32, False)):
        rcv, msgs, recs = make_list(np, A, n, R, seed=11 + R)
        cfg = dict(seconds_per_tick=1e-9, use_altitude=alt)
        dm = torch.from_numpy(msgs.view(np.uint8).reshape(-1)).cuda()
        dr = torch.from_numpy(recs.view(np.uint8).reshape(-1)).cuda()
        lists = ((dm.data_ptr(), n), (dr.data_ptr(), len(recs)))
        got, hdr = dem.multilaterate_of(rcv, *lists, **cfg)
        t0 = time.perf_counter()
        want, _ = A.host_multilaterate(rcv, msgs, recs, **cfg)
        host_us = (time.perf_counter() - t0) * 1e6
        same = int((got["flags"] == want["flags"]).sum())
        both = (got["flags"] & want["flags"] & A.ADSB_MLAT_VALID) != 0
        gap = float(np.abs(np.stack([got[k][both] - want[k][both] for k in ("latitude", "longitude")])).max()) if both.any() else 0.0
        t = timed(lambda: dem.multilaterate_of_async(rcv, *lists, **cfg))
        lines.append(f"{name:22s} {t[0]:9.1f} us (min {t[1]:.1f}, max {t[2]:.1f}, {args.reps} reps); "
                     f"{int(hdr['n_valid'])} of {n} valid, {float(got['iterations'].mean()):.1f} steps per message; "
                     f"adsb_host_multilaterate on one CPU core: {host_us:.0f} us; flags equal for {same} of {n}, "
                     f"largest |lat/lon| difference over fixes valid in both {gap:.3g} deg\n")
        del dm, dr
    dem.close()
    text = (f"multilaterate (adsb_multilaterate_of, lists in device memory), device time per call, median over the "
            f"repetitions\n{n} messages, 1 ns ticks\n" + "".join(lines))
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
