#!/usr/bin/env python3
"""GPU box helper: what the filter behind a table's multilaterated fixes (adsb_track_table_filter_reserve) adds to
adsb_track_table_update_mlat, measured with device events on the ctx stream around the whole update, warm, medians with
their range.

Three lists, frames and fixes in device memory, every fix valid and usable, into tables that already hold every aircraft
(one untimed update first, so no timed update admits anything); every round moves the sample base on by a second, so every
frame is APPLIED (a list fed twice at one base would be SKIPPED frames, which cost nothing):
  a. 64 frames of 8 aircraft: the two dispatches' own cost;
  b. 32 768 frames of 2 048 aircraft, the size tools/gpu/track_mlat_timing.py merges: 16 frames a walk;
  c. 32 768 frames of ONE aircraft: the walk's worst case, one lane stepping through the whole list.
For each, in ALTERNATING runs: update_mlat on a table with the mlat reserve only, and on one with the filter reserve too.
The library is whichever ADSB_HIP_LIB names (with ADSB_HIP_LIB_LENIENT=1 for a build without the filter entry points,
e.g. the parent commit's: then only the table without the filter reserve is measured), so one GPU call can alternate
builds in processes of their own: "a table that never reserves is unaffected" rests on the parent's figure and this
build's agreeing within what two passes of one build differ by.  `--label` names the pass; `--out PATH` appends the
report to PATH (a run is meant to be kept as profiles/track_filter_timing.txt)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import air_rs_amd as A
from air_rs_amd import _lib as L

ap = argparse.ArgumentParser()
ap.add_argument("--out", help="append the report to this file")
ap.add_argument("--label", default="this build")
ap.add_argument("--reps", type=int, default=30)
ap.add_argument("--warmup", type=int, default=4)
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


def make_list(n, n_aircraft, seed):
    """n identification frames in ascending offset (20 us apart) and a valid fix for each, within 20 m of its aircraft's
    place: every frame is usable and none is an outlier."""
    rng = np.random.default_rng(seed)
    lat0, lon0 = 47.0 + rng.uniform(-1, 1, n_aircraft), 8.0 + rng.uniform(-1.5, 1.5, n_aircraft)
    who = rng.integers(0, n_aircraft, n)
    frames = np.zeros(n, dtype=A.FRAME_DTYPE)
    frames["offset"] = 100 + 40 * np.arange(n)
    icao = 0x400000 + who
    frames["bytes"][:, 0] = 0x8D
    for k in range(3):
        frames["bytes"][:, 1 + k] = (icao >> (16 - 8 * k)) & 0xFF
    frames["bytes"][:, 4] = 4 << 3
    frames["fixed_bit"] = 0xFF
    fixes = np.zeros(n, dtype=A.MLAT_FIX_DTYPE)
    fixes["latitude"] = lat0[who] + rng.uniform(-1.8e-4, 1.8e-4, n)
    fixes["longitude"] = lon0[who] + rng.uniform(-2.6e-4, 2.6e-4, n)
    fixes["height_m"] = 9000.0 + rng.uniform(-20, 20, n)
    fixes["residual_rms_m"], fixes["pdop"], fixes["hdop"], fixes["vdop"], fixes["n_used"] = 5.0, 2.9, 1.5, 2.5, 6
    fixes["flags"] = 0x1 | 0x2 | 0x100
    return frames, fixes


torch.cuda.set_stream(torch.cuda.Stream())  # a stream of our own: a NULL stream would make the ctx create one
stream = torch.cuda.current_stream().cuda_stream
HAVE = hasattr(L.load(), "adsb_track_table_filter_reserve")
say(f"==== {args.label}: device {torch.cuda.get_device_name(0)}"
    f"{'' if HAVE else ' (no filter entry points: update_mlat without the filter reserve only)'}")
dem = A.AdsbDemod(device=0, stream=stream, host_staging=False, max_samples=1 << 16, max_out=1024)
for name, n, n_aircraft in (("a. 64 frames of 8 aircraft", 64, 8), ("b. 32768 frames of 2048 aircraft", 32768, 2048),
                            ("c. 32768 frames of 1 aircraft", 32768, 1)):
    frames, fixes = make_list(n, n_aircraft, seed=n + n_aircraft)
    df = torch.from_numpy(frames.view(np.uint8).reshape(-1)).cuda()
    dx = torch.from_numpy(fixes.view(np.uint8).reshape(-1)).cuda()
    kw = dict(max_aircraft=4096, max_frames=n, seconds_per_sample=0.5e-6)
    with A.TrackTable(dem, **kw) as plain, A.TrackTable(dem, **kw) as table:
        plain.mlat_reserve(1000.0)
        calls = {"update_mlat, mlat reserve only": plain}
        if HAVE:
            table.mlat_reserve(1000.0)
            table.filter_reserve()
            calls["update_mlat, filter reserve too"] = table
        got = {k: [] for k in calls}
        for rep in range(args.warmup + args.reps):       # alternating: one of each per round
            base = 2_000_000 * rep
            for k, t in calls.items():
                x = timed_ms(lambda: t.update_device(df.data_ptr(), n, base, mlat_ptr=dx.data_ptr()))
                if rep >= args.warmup:
                    got[k].append(x)
        say(f"{name}, frames and fixes in device memory, device time of one update ({args.reps} alternating rounds):")
        for k in calls:
            say(f"  {k:32s} {stats(got[k])}")
        if HAVE:
            f = table.filter()
            rounds = args.warmup + args.reps
            assert len(f) == n_aircraft and int(f["n_applied"].sum()) == n * rounds - n_aircraft, f["n_applied"].sum()
            assert int(f["n_outlier"].sum()) == int(f["n_skipped"].sum()) == int(f["n_reset"].sum()) == 0
            a, b = got["update_mlat, mlat reserve only"], got["update_mlat, filter reserve too"]
            d = np.array(b) - np.array(a)                # one pair per round
            say(f"  the filter adds {1e3 * np.median(d):.1f} us (rounds' differences: min {1e3 * d.min():.1f}, max "
                f"{1e3 * d.max():.1f}), {1e6 * np.median(d) / n:.3f} ns per frame; longest walk "
                f"{int(np.bincount(frames['bytes'][:, 3].astype(np.int64) | frames['bytes'][:, 2].astype(np.int64) << 8).max())} frames")
    del df, dx
dem.close()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as fh:
        fh.write("\n".join(lines) + "\n")
