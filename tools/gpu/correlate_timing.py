#!/usr/bin/env python3
"""GPU box helper: device time of correlate (adsb_correlate_of: the key kernel, rocPRIM's merge sort, the aggregate scan,
the radix sort by group time, the head-mark scan and the write kernel) for a 64-receiver list of 65 536 frames that is
already in device memory with its level records, measured with device events on the ctx stream, one process.  The
events enclose the whole call, the copy of the 65 receiver prefixes and 64 bases and the wait for it included (the six
steps themselves are enqueued without the host reading anything back).

  tools/gpu/correlate_timing.py --out profiles/correlate_timing.txt

The list: about a third as many transmissions as receptions, each heard by random receivers a few samples apart, so
groups of one to a dozen receptions occur; and, as the other extreme, the same number of identical frames (one group).
The result of the first repetition is compared with the CPU mirror's, byte for byte.  Under a kernel trace
(rocprofv3 --kernel-trace --stats -- python tools/gpu/correlate_timing.py --reps 20) the steps' own times appear as
corr_keys, corr_write and rocPRIM's kernels."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def make_list(np, A, n, n_receivers, seed, one_group=False):
    """(frames, counts, levels): receiver-major, ascending offset per receiver."""
    rng = np.random.default_rng(seed)
    n_tx = 1 if one_group else max(n // 3, 1)
    tx_bytes = rng.integers(0, 256, size=(n_tx, 14)).astype(np.uint8)
    tx_time = np.cumsum(rng.integers(200, 4000, size=n_tx)).astype(np.uint64)
    tx = rng.integers(0, n_tx, size=n)
    rx = rng.integers(0, n_receivers, size=n)
    t = tx_time[tx] + rng.integers(0, 60, size=n).astype(np.uint64)
    order = np.lexsort((t, rx))
    fr = np.zeros(n, dtype=A.FRAME_DTYPE)
    fr["offset"], fr["bytes"] = t[order], tx_bytes[tx[order]]
    fr["status"] = rng.integers(0, 2, size=n)
    fr["fixed_bit"] = np.where(fr["status"] == 1, rng.integers(0, 88, size=n), 0xFF)
    lv = np.zeros(n, dtype=A.LEVEL_DTYPE)
    lv["signal_sum"] = rng.integers(0, 1 << 20, size=n)
    lv["flags"] = (rng.integers(0, 16, size=n) != 0).astype(np.uint16)
    counts = np.bincount(rx, minlength=n_receivers).astype(np.uint64)
    return fr, counts, lv


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=65536)
    ap.add_argument("--receivers", type=int, default=64)
    ap.add_argument("--window", type=int, default=100)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", help="also write the report to this file")
    args = ap.parse_args()

    import numpy as np
    import torch

    import air_rs_amd as A

    n, R = args.frames, args.receivers
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
    for name, one_group in (("mixed groups", False), ("one group", True)):
        fr, counts, lv = make_list(np, A, n, R, seed=7, one_group=one_group)
        base = np.arange(R, dtype=np.uint64) * 3
        window = args.window if not one_group else 1 << 31
        dfr = torch.from_numpy(fr.view(np.uint8).reshape(-1)).cuda()
        dlv = torch.from_numpy(lv.view(np.uint8).reshape(-1)).cuda()
        got = dem.correlate_of((dfr.data_ptr(), n), counts, window, base, dlv.data_ptr())
        t0 = time.perf_counter()
        want = A.host_correlate(fr, counts, window, base, lv)
        host_us = (time.perf_counter() - t0) * 1e6
        assert all(g.tobytes() == w.tobytes() for g, w in zip(got, want)), "device result != CPU mirror's"
        t = timed(lambda: dem.correlate_of_async((dfr.data_ptr(), n), counts, window, base, dlv.data_ptr()))
        lines.append(f"{name:14s} {t[0]:8.1f} us (min {t[1]:.1f}, max {t[2]:.1f}, {args.reps} reps); {len(got[0])} messages, "
                     f"longest group {int(got[0]['n_receptions'].max())}; adsb_host_correlate on one CPU core: {host_us:.0f} us\n")
        del dfr, dlv
    dem.close()
    text = (f"correlate (adsb_correlate_of, lists in device memory), device time per call, median over the repetitions\n"
            f"{R} receivers, {n} frames with levels\n" + "".join(lines)
            + "the device results equal the CPU mirror's byte for byte\n")
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
