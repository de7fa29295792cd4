#!/usr/bin/env python3
"""GPU box helper: cost of the fused view of a track bank (adsb_track_bank_fuse: key kernel + rocPRIM radix sort + scan of
the ICAO changes + one reduction per ICAO), measured with device events on the ctx stream, next to what bounds it and to
the path a user had before it.

  1. a full bank of 64 receivers x 65 536 aircraft with EVERY aircraft on every receiver (65 536 fused records from runs
     of 64 records) and the same bank with DISJOINT ICAO sets (4 Mi fused records from runs of one): device us per fuse
     for each number of lanes per ICAO the reduction can use (ADSB_FUSE_LANES, read by fuse_reserve; the first one listed
     is the library's choice), and from the same run adsb_time_read_ceiling over 128 bytes x places (the least any fusion
     must read) and the bank's expire evicting nothing (one pass over all records with one scan);
  2. the path without it on the same banks, wall clock: the three fetches (aircraft(), last_heard(), velocity()) and a
     vectorised NumPy merge by the header's rules, whose output is compared with the device's byte for byte;
  3. small banks, where the fixed cost of the dispatch sequence shows: 64 receivers holding 35 aircraft each, in a bank
     with 65 536 places per receiver (the sort still runs over every place) and in one with 64.
Prints the report; `--out PATH` also writes it to PATH (profiles/track_bank_fuse_timing.txt holds a run)."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import air_rs_amd as A

ap = argparse.ArgumentParser()
ap.add_argument("--out", help="also write the report to this file")
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--receivers", type=int, default=64)
ap.add_argument("--aircraft", type=int, default=65536, help="places per receiver of the full banks")
ap.add_argument("--skip-host", action="store_true", help="leave out the host path (2.)")
args = ap.parse_args()
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed_ms(fn):
    """device ms of fn() alone (everything enqueued before it has finished first)"""
    st = torch.cuda.current_stream()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record(st)
    fn()
    b.record(st)
    b.synchronize()
    return a.elapsed_time(b)


def frames_of(icaos, kind):
    """one frame per ICAO, offsets 0, 1, 2, ... (the tracker reads the fields only; the CRC is not looked at):
    kind 0 an identification (TC 4), kind 1 an airborne velocity (TC 19 ST 1, 100 kt east and north)"""
    f = np.zeros(len(icaos), dtype=A.FRAME_DTYPE)
    b = np.zeros((len(icaos), 14), dtype=np.uint8)
    b[:, 0] = 0x8D
    b[:, 1], b[:, 2], b[:, 3] = (icaos >> 16) & 0xFF, (icaos >> 8) & 0xFF, icaos & 0xFF
    if kind == 0:
        b[:, 4] = 4 << 3
        b[:, 5:11] = 0x41
    else:
        me = 19 << 51 | 1 << 48 | 101 << (56 - 14 - 10) | 101 << (56 - 25 - 10)
        b[:, 4:11] = np.frombuffer(me.to_bytes(7, "big"), dtype=np.uint8)
    f["bytes"] = b
    f["offset"] = np.arange(len(icaos))
    f["fixed_bit"] = 0xFF
    return f


def stats(xs):
    return f"{1e3 * np.median(xs):9.1f} us (min {1e3 * min(xs):.1f}, max {1e3 * max(xs):.1f})"


def host_merge(recs, heard, vel):
    """The header's rules over the three fetches, vectorised: one stable sort by ICAO (receivers stay ascending inside a
    run), per quantity the first record of each run that reaches the run's greatest time."""
    rcv = np.concatenate([np.full(len(x), r, dtype=np.uint16) for r, x in enumerate(recs)])
    rec, lh, v = np.concatenate(recs), np.concatenate(heard), np.concatenate(vel)
    order = np.argsort(rec["icao"], kind="stable")
    rec, lh, v, rcv = rec[order], lh[order], v[order], rcv[order]
    n = len(rec)
    head = np.flatnonzero(np.concatenate([[True], rec["icao"][1:] != rec["icao"][:-1]])) if n else np.zeros(0, np.int64)
    out = np.zeros(len(head), dtype=A.FUSED_DTYPE)
    if not n:
        return out
    pos = np.arange(n)

    def winner(t, has):
        key = np.where(has, t, -np.inf)
        best = np.maximum.reduceat(key, head)
        seg = np.searchsorted(head, pos, side="right") - 1
        hit = has & (key == best[seg])
        first = np.minimum.reduceat(np.where(hit, pos, n), head)
        return first, first < n

    out["icao"] = rec["icao"][head]
    out["n_receivers"] = np.add.reduceat(np.ones(n, dtype=np.int64), head)
    out["n_frames"] = np.add.reduceat(rec["n_frames"].astype(np.uint64), head)
    for name in ("contact_receiver", "position_receiver", "callsign_receiver", "velocity_receiver"):
        out[name] = A.ADSB_FUSED_NONE
    out["last_contact"] = out["position_time"] = np.nan
    out["velocity"]["time"] = np.nan
    w, ok = winner(lh, np.ones(n, dtype=bool))
    out["heard_receiver"], out["last_heard"] = rcv[w], lh[w]
    w, ok = winner(rec["last_contact"], ~np.isnan(rec["last_contact"]))
    w = w[ok]
    out["contact_receiver"][ok], out["last_contact"][ok], out["altitude"][ok] = rcv[w], rec["last_contact"][w], rec["altitude"][w]
    w, ok = winner(rec["last_contact"], rec["has_position"] != 0)
    w = w[ok]
    out["position_receiver"][ok], out["has_position"][ok] = rcv[w], 1
    out["latitude"][ok], out["longitude"][ok] = rec["latitude"][w], rec["longitude"][w]
    out["position_time"][ok] = rec["last_contact"][w]
    w, ok = winner(lh, rec["callsign"] != b"")
    w = w[ok]
    out["callsign_receiver"][ok], out["callsign"][ok] = rcv[w], rec["callsign"][w]
    w, ok = winner(v["time"], v["subtype"] != 0)
    w = w[ok]
    out["velocity_receiver"][ok] = rcv[w]
    vout = out["velocity"]
    vout[ok] = v[w]
    out["velocity"] = vout
    return out


torch.cuda.set_stream(torch.cuda.Stream())  # a stream of our own: a NULL stream would make the ctx create one
stream = torch.cuda.current_stream().cuda_stream
say(f"device {torch.cuda.get_device_name(0)}")
rng = np.random.default_rng(1)
M, R, sps = args.aircraft, args.receivers, 1e-3
places = R * M
all_icaos = rng.choice(np.arange(0, 1 << 24), size=places, replace=False).astype(np.uint32)  # order unrelated to ICAO
default_lanes = 1 if R == 1 else 4
lane_list = [default_lanes] + [g for g in (1, 4) if g != default_lanes]


def fill(bank, disjoint):
    """every receiver hears M aircraft twice: an identification, then a velocity; receiver r's clock is 1000 r ahead"""
    for kind in (0, 1):
        lists = [frames_of(all_icaos[r * M:(r + 1) * M] if disjoint else all_icaos[:M], kind) for r in range(R)]
        bank.update(np.concatenate(lists), [M] * R, [kind * 2 * M + 1000 * r for r in range(R)])


reserved = 0  # bytes the bank's current reserve holds


def measure(bank, what, max_fused, want_records, ceiling_buf, dem):
    global reserved
    say(f"{what}:")
    free0 = torch.cuda.mem_get_info()[0] + reserved  # as if the previous reserve had been given back first
    for g in lane_list:
        os.environ["ADSB_FUSE_LANES"] = str(g)
        bank.fuse_reserve(max_fused)
        if g == lane_list[0]:
            reserved = free0 - torch.cuda.mem_get_info()[0]
            say(f"  fuse_reserve(max_fused = {max_fused}): {reserved / 2**20:.1f} MiB of device memory")
        ms = [timed_ms(bank.fuse_async) for _ in range(args.reps + 2)]
        say(f"  fuse, {g:2d} lane{'s' if g > 1 else ' '} per ICAO{' (the choice)' if g == lane_list[0] else '':13s}: {stats(ms[2:])}")
    del os.environ["ADSB_FUSE_LANES"]
    bank.fuse_reserve(max_fused)
    bank.fuse_async()
    ptr, counts = bank.fused_device()
    ms = [timed_ms(lambda: bank.expire(-1.0)) for _ in range(args.reps + 1)]
    say(f"  expire evicting 0 % of the same bank:        {stats(ms[1:])}")
    nbytes = 128 * places
    ms = dem.time_read_ceiling(ceiling_buf.data_ptr(), nbytes, 10)
    say(f"  read ceiling over 128 B x {places} places ({nbytes / 2**20:.0f} MiB): {1e3 * ms:9.1f} us ({nbytes / ms / 1e9:.2f} TB/s)")
    if args.skip_host:
        return
    t0 = time.perf_counter()
    recs, _ = bank.aircraft()
    heard = bank.last_heard()
    vel = bank.velocity()
    t1 = time.perf_counter()
    merged = host_merge(recs, heard, vel)
    t2 = time.perf_counter()
    fused, total, flags = bank.fuse()
    t3 = time.perf_counter()
    assert total == want_records == len(fused) and flags == 0, (total, want_records, len(fused), flags)
    assert merged.tobytes() == fused.tobytes(), "the host merge and the device disagree"
    fuse_ms = np.median([timed_ms(bank.fuse_async) for _ in range(3)])
    say(f"  without it, wall clock: aircraft() + last_heard() + velocity() {t1 - t0:7.2f} s, NumPy merge {t2 - t1:6.2f} s"
        f" = {t2 - t0:.2f} s  ({1e3 * (t2 - t0) / fuse_ms:.0f} x the fuse on the device;"
        f" fuse + fetch of {len(fused)} records, wall clock: {t3 - t2:.3f} s); outputs equal byte for byte")


# ---- 1. / 2. full banks ---------------------------------------------------------------------------------------------
ceiling_buf = torch.zeros(128 * places, dtype=torch.uint8, device="cuda")
dem = A.AdsbDemod(device=0, max_samples=1 << 16, max_out=1 << 12, stream=stream, host_staging=False)
with A.TrackBank(dem, R, max_aircraft=M, max_frames=places, seconds_per_sample=sps) as bank:
    fill(bank, disjoint=False)
    measure(bank, f"bank, {R} receivers x {M} aircraft, full, every aircraft on every receiver ({M} fused records)", M, M,
            ceiling_buf, dem)
    bank.reset()
    fill(bank, disjoint=True)
    measure(bank, f"the same bank, disjoint ICAO sets ({places} fused records)", 0, places, ceiling_buf, dem)
dem.close()

# ---- 3. small banks -------------------------------------------------------------------------------------------------
for max_ac in (M, 64):
    dem = A.AdsbDemod(device=0, max_samples=1 << 16, max_out=1 << 12, stream=stream, host_staging=False)
    with A.TrackBank(dem, R, max_aircraft=max_ac, max_frames=1 << 14, seconds_per_sample=sps) as bank:
        few = frames_of(all_icaos[:35], 0)
        bank.update(np.concatenate([few] * R), [35] * R, [10 * r for r in range(R)])
        bank.fuse_reserve(4096)
        ms = [timed_ms(bank.fuse_async) for _ in range(50)]
        fused, total, flags = bank.fuse()
        assert total == 35 and (fused["n_receivers"] == R).all()
        say(f"small bank, {R} receivers holding 35 aircraft each, {max_ac} places per receiver: fuse {stats(ms[5:])}")
        ms = [timed_ms(lambda: bank.expire(-1.0)) for _ in range(50)]
        say(f"  expire evicting 0 % of the same bank:        {stats(ms[5:])}")
    dem.close()

if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
