#!/usr/bin/env python3
"""GPU box helper: what the per-frame summaries and the changed list (adsb_track_*_summaries_reserve) cost, measured
with device events on the ctx stream, warm, medians and ranges, next to the same update without a reserve.

  a. small lists: a table fed 1 / 8 / 64 frames per update, a bank of 64 receivers fed 1 / 32 frames per receiver;
  b. the config-4 list (64 channels x 8 Mi samples of synthetic i8 in one launch, ~253 k frames, every frame its own
     ICAO) through a bank's update_launch, and a list of 65 536 frames of ONE aircraft (0.1 s apart) through a table:
     update without a reserve, with one, the difference per frame, and the read ceiling of the same run over 256 bytes
     per frame (about what the two new steps move: they read ~200 bytes per frame and write 72);
  c. fetch_changed against aircraft() + last_heard() + velocity() on a full table of 65 536 aircraft after an update
     of 64 frames, wall clock (the point is the copy and the host sort avoided).
The library is whichever ADSB_HIP_LIB names (with ADSB_HIP_LIB_LENIENT=1 for a build without the summaries entry
points, e.g. the parent commit's: then only the updates without a reserve are measured), so one GPU call can alternate
builds.  `--label` names the pass; `--out PATH` appends the report to PATH (profiles/track_summaries_timing.txt holds a
run).  `--trace small|config4|one-aircraft [--reserve]` runs only that update loop, for a rocprofv3 --kernel-trace
--stats run of its own, and `--kernel-stats LABEL DIR` (repeatable, no GPU needed) adds such a run's per-kernel table
to the report; tools/gpu/track_summaries_timing.sh strings the passes together."""
import argparse
import csv
import glob
import re
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import air_rs_amd as A
from air_rs_amd import _lib as L
from tests.oracle_binding import Oracle
from tests.traffic import random_traffic

ap = argparse.ArgumentParser()
ap.add_argument("--out", help="append the report to this file")
ap.add_argument("--label", default="this build")
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--trace", choices=["small", "config4", "one-aircraft"],
                help="only run this update loop (for a kernel trace)")
ap.add_argument("--reserve", action="store_true", help="with --trace: reserve the summaries first")
ap.add_argument("--kernel-stats", nargs=2, action="append", metavar=("LABEL", "DIR"),
                help="only report the tracker's kernels from a rocprofv3 --kernel-trace --stats output directory")
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


def stats(xs):
    return f"{1e3 * np.median(xs):9.1f} us (min {1e3 * min(xs):.1f}, max {1e3 * max(xs):.1f})"


def pool_of(oracle, seed, n_aircraft, n_frames):
    traffic = random_traffic(oracle, seed=seed, n_aircraft=n_aircraft, n_frames=n_frames)
    pool = np.zeros(len(traffic), dtype=A.FRAME_DTYPE)
    pool["bytes"] = np.array([np.frombuffer(fr, dtype=np.uint8) for _, fr in traffic])
    pool["fixed_bit"] = 0xFF
    return pool


def new_dem(**kw):
    kw.setdefault("max_samples", 1 << 16)
    kw.setdefault("max_out", 1 << 12)
    return A.AdsbDemod(device=0, stream=stream, host_staging=False, **kw)


def finish():
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")
    sys.exit(0)


def kernel_name(name):
    """a traced kernel's name, short; None for kernels that are not the tracker's"""
    sums = " <TrackSumTuple>" if "TrackSumTuple" in name else ""
    if "init_lookback_scan_state" in name:
        return "rocprim init_lookback_scan_state" + sums
    m = re.search(r"wrapped_(\w+?)_config", name)
    if m:
        return "rocprim " + m.group(1) + sums
    m = re.search(r"(track_\w+(?:<\w+>)?|decode_fields_kernel)", name)
    return m.group(1) if m else None


if args.kernel_stats:
    for label, path in args.kernel_stats:
        say(f"==== kernel trace, {label}: kernel, calls, average ns")
        found = glob.glob(os.path.join(path, "**", "*kernel_stats.csv"), recursive=True)
        agg = {}
        for row in csv.DictReader(open(found[0])):
            k = kernel_name(row["Name"])
            if k:
                c, t = agg.get(k, (0, 0))
                agg[k] = (c + int(row["Calls"]), t + int(row["TotalDurationNs"]))
        for k, (c, t) in sorted(agg.items()):
            say(f"  {k:48s} {c:5d} {t / c:10.0f}")
    finish()

torch.cuda.set_stream(torch.cuda.Stream())  # a stream of our own: a NULL stream would make the ctx create one
stream = torch.cuda.current_stream().cuda_stream
oracle = Oracle()
HAVE = hasattr(L.load(), "adsb_track_table_summaries_reserve")
say(f"==== {args.label}: device {torch.cuda.get_device_name(0)}"
    f"{'' if HAVE else ' (no summaries entry points: updates without a reserve only)'}")
variants = [False, True] if HAVE else [False]
sps_small = 1.0 / 20000


def small_table(reserve, k, reps):
    pool = pool_of(oracle, 500, 35, 600)
    dem = new_dem()
    with A.TrackTable(dem, max_frames=64, seconds_per_sample=sps_small) as t:
        if reserve:
            t.summaries_reserve()
        step = [0]

        def one():
            u = step[0]
            x = pool[(u * k) % (len(pool) - k):][:k].copy()
            x["offset"] = 300 + 300 * np.arange(k)
            t.update(x, 20000 * u)
            step[0] += 1

        for _ in range(40):
            one()
        ms = [timed_ms(one) for _ in range(reps)]
    dem.close()
    return ms


def small_bank(reserve, k, reps, R=64):
    pools = [pool_of(oracle, 1000 + r, 35, 300) for r in range(R)]
    dem = new_dem()
    with A.TrackBank(dem, R, max_frames=R * 32, seconds_per_sample=sps_small) as b:
        if reserve:
            b.summaries_reserve()
        step = [0]

        def one():
            u = step[0]
            parts = []
            for r in range(R):
                x = pools[r][(u * k) % (len(pools[r]) - k):][:k].copy()
                x["offset"] = 300 + 300 * np.arange(k)
                parts.append(x)
            b.update(np.concatenate(parts), [k] * R, [20000 * u + 11 * r for r in range(R)])
            step[0] += 1

        for _ in range(20):
            one()
        ms = [timed_ms(one) for _ in range(reps)]
    dem.close()
    return ms


def one_aircraft_list(n=1 << 16, step=100):
    palette = pool_of(oracle, 61, 1, 512)
    frames = palette[np.random.default_rng(61).integers(0, len(palette), size=n)].copy()
    frames["offset"] = np.arange(n, dtype=np.uint64) * step
    return frames


def big_single(reserve, reps):
    """65 536 frames of one aircraft, in device memory (no copy in the timed part)"""
    frames = one_aircraft_list()
    n = len(frames)
    dev = torch.from_numpy(frames.view(np.uint8).copy()).cuda()
    dem = new_dem()
    ceiling = torch.zeros(256 * n, dtype=torch.uint8, device="cuda")
    with A.TrackTable(dem, max_aircraft=16, max_frames=n, seconds_per_sample=1e-3) as t:
        if reserve:
            t.summaries_reserve()
        base = [0]

        def one():
            base[0] += n * 100
            t.update_device(dev.data_ptr(), n, base[0])

        for _ in range(2):
            one()
        ms = [timed_ms(one) for _ in range(reps)]
        ceil_ms = dem.time_read_ceiling(ceiling.data_ptr(), 256 * n, 10)
    dem.close()
    return ms, n, ceil_ms


class Config4:
    """the config-4 launch, kept for both variants"""

    def __init__(self, R=64):
        n = 1 << 29
        self.R, self.n_ch = R, (n // R) & ~7
        cfg = A.synth_default()
        self.cap = n // cfg.slot_len + 8192
        self.iq = torch.empty(n * 2, dtype=torch.int8, device="cuda")
        self.dem = new_dem(max_samples=self.n_ch, max_out=self.cap, max_channels=R)
        for c in range(R):
            self.dem.synth_fill_device(cfg, c, 0, self.n_ch, self.iq.data_ptr() + c * self.n_ch * 2)
        self.dem.demod_device_async(self.iq.data_ptr(), self.n_ch, n_channels=R, channel_stride=self.n_ch)
        self.n_out, _, _ = self.dem.fetch_counts()

    def run(self, reserve, reps):
        with A.TrackBank(self.dem, self.R, max_frames=self.cap, seconds_per_sample=0.5e-6) as b:
            if reserve:
                b.summaries_reserve()
            base = [0]

            def again():
                base[0] += self.n_ch
                b.update_launch([base[0]] * self.R)

            for _ in range(2):
                again()                     # the bank now holds every ICAO
            return [timed_ms(again) for _ in range(reps)]

    def ceiling(self):
        buf = torch.zeros(256 * self.n_out, dtype=torch.uint8, device="cuda")
        return self.dem.time_read_ceiling(buf.data_ptr(), 256 * self.n_out, 10)


if args.trace:
    if args.trace == "small":
        small_table(args.reserve, 64, 20)
    elif args.trace == "config4":
        Config4().run(args.reserve, 3)
    else:
        big_single(args.reserve, 3)
    sys.exit(0)

# ---- a. small lists -------------------------------------------------------------------------------------------------
say("a. small lists (host frames, 35 aircraft per receiver), device us per update:")
for what, fn, sizes in (("table, frames", small_table, (1, 8, 64)),
                        ("bank of 64 receivers, frames per receiver", small_bank, (1, 32))):
    for k in sizes:
        got = {r: fn(r, k, args.reps) for r in variants}
        line = f"  {what} {k:3d}: without a reserve {stats(got[False])}"
        if HAVE:
            line += f"; with one {stats(got[True])}; added {1e3 * (np.median(got[True]) - np.median(got[False])):.1f} us"
        say(line)

# ---- b. long lists --------------------------------------------------------------------------------------------------
c4 = Config4()
got = {r: c4.run(r, 7) for r in variants}
ceil_ms = c4.ceiling()
say(f"b. config 4 through update_launch ({c4.n_out} frames, {c4.R} receivers, the bank holds every ICAO), device time:")
line = f"  without a reserve {stats(got[False])}"
added_c4 = None
if HAVE:
    added_c4 = 1e6 * (np.median(got[True]) - np.median(got[False])) / c4.n_out
    line += f"; with one {stats(got[True])}; added {added_c4:.3f} ns per frame"
say(line)
say(f"  read ceiling over 256 B x {c4.n_out} frames: {1e3 * ceil_ms:.1f} us ({256 * c4.n_out / ceil_ms / 1e9:.2f} TB/s)")
del c4
res = {r: big_single(r, 7) for r in variants}
n1 = res[False][1]
say(f"   one aircraft, {n1} frames 0.1 s apart in one table update (device list), device time:")
line = f"  without a reserve {stats(res[False][0])}"
if HAVE:
    added_1 = 1e6 * (np.median(res[True][0]) - np.median(res[False][0])) / n1
    line += f"; with one {stats(res[True][0])}; added {added_1:.3f} ns per frame (config 4: {added_c4:.3f})"
say(line)
say(f"  read ceiling over 256 B x {n1} frames: {1e3 * res[False][2]:.1f} us")

# ---- c. fetch_changed against the three fetches on a full table --------------------------------------------------------
if HAVE:
    M = 65536
    icaos = np.random.default_rng(3).choice(np.arange(0, 1 << 24), size=M, replace=False).astype(np.uint32)
    fill = np.zeros(M, dtype=A.FRAME_DTYPE)
    fb = np.zeros((M, 14), dtype=np.uint8)
    fb[:, 0], fb[:, 1], fb[:, 2], fb[:, 3], fb[:, 4] = 0x8D, (icaos >> 16) & 0xFF, (icaos >> 8) & 0xFF, icaos & 0xFF, 4 << 3
    fb[:, 5:11] = 0x41
    fill["bytes"], fill["offset"], fill["fixed_bit"] = fb, np.arange(M), 0xFF
    dem = new_dem()
    with A.TrackTable(dem, max_aircraft=M, max_frames=M, seconds_per_sample=1e-3) as t:
        t.summaries_reserve()
        t.update(fill)
        few = fill[:64].copy()
        t_changed, t_three = [], []
        for u in range(12):
            t.update(few, M + 100 * u)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            recs, heard, vel = t.changed()
            t1 = time.perf_counter()
            all_recs, all_heard, all_vel = t.aircraft()[0], t.last_heard(), t.velocity()
            t2 = time.perf_counter()
            rows = np.searchsorted(all_recs["icao"], recs["icao"])
            assert len(recs) == 64 and recs.tobytes() == all_recs[rows].tobytes()
            assert heard.tobytes() == all_heard[rows].tobytes() and vel.tobytes() == all_vel[rows].tobytes()
            t_changed.append(1e3 * (t1 - t0))
            t_three.append(1e3 * (t2 - t1))
    dem.close()
    say(f"c. full table of {M} aircraft, after an update of 64 frames, wall clock (Python calls included):")
    say(f"  changed(): {stats(t_changed[2:])}; aircraft() + last_heard() + velocity(): {stats(t_three[2:])};"
        f" same 64 rows byte for byte")

finish()
