#!/usr/bin/env python3
"""GPU box helper: what the per-aircraft mlat merge (adsb_track_table_mlat_reserve, adsb_track_table_update_mlat) costs,
measured with device events on the ctx stream around the update alone, warm, medians with their range.

Two lists, frames and fixes in device memory, into a table that already holds every aircraft (one untimed update first,
so no timed update admits anything):
  a. 64 frames of 8 aircraft: the dispatches' own cost;
  b. 32 768 frames of 2 048 aircraft, the size tools/gpu/mlat_timing.py solves: three in four are airborne position
     messages with a valid fix, so three in four frames run the CPR decode and the haversine.
For each, in ALTERNATING runs on one table: `update` and `update_mlat`, and `update` on a table without the reserve.
The library is whichever ADSB_HIP_LIB names (with ADSB_HIP_LIB_LENIENT=1 for a build without the mlat entry points, e.g.
the parent commit's: then only `update` without a reserve is measured), so one GPU call can alternate builds: "a table
that never reserves is unaffected" rests on the parent's figure and this build's agreeing within the run-to-run spread
the same report shows.  `--label` names the pass; `--out PATH` appends the report to PATH (a run is meant to be kept as
profiles/track_mlat_timing.txt)."""
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
ap.add_argument("--reps", type=int, default=40)
ap.add_argument("--warmup", type=int, default=5)
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


def cpr(lat, lon, odd):
    """DO-260's airborne encoder, vectorised (NL from the closed form; exact zone edges do not matter here)."""
    d_lat = 360.0 / (60 - odd)
    yz = np.floor(131072.0 * np.mod(lat, d_lat) / d_lat + 0.5)
    rlat = d_lat * (yz / 131072.0 + np.floor(lat / d_lat))
    a = 1.0 - np.cos(np.pi / 30.0)
    nl = np.floor(2.0 * np.pi / np.arccos(1.0 - a / np.cos(np.radians(rlat)) ** 2))
    d_lon = 360.0 / np.maximum(nl - odd, 1)
    xz = np.floor(131072.0 * np.mod(lon, d_lon) / d_lon + 0.5)
    return yz.astype(np.uint64) & 0x1FFFF, xz.astype(np.uint64) & 0x1FFFF


def make_list(n, n_aircraft, seed):
    """n frames in ascending offset and a fix for each: 3 in 4 airborne position messages (one in ten of them 5 km off)
    with a valid fix at the aircraft's place, the rest velocity messages with a fix that was not attempted."""
    rng = np.random.default_rng(seed)
    lat0, lon0 = 47.0 + rng.uniform(-1, 1, n_aircraft), 8.0 + rng.uniform(-1.5, 1.5, n_aircraft)
    who = rng.integers(0, n_aircraft, n)
    pos = rng.random(n) < 0.75
    odd = rng.integers(0, 2, n).astype(np.uint64)
    lat = lat0[who] + np.where(rng.random(n) < 0.1, 0.045, 0.0)
    yz, xz = cpr(lat, lon0[who], odd.astype(np.float64))
    me = np.where(pos, np.uint64(11) << np.uint64(51) | np.uint64(0x3A8) << np.uint64(36) | odd << np.uint64(34) |
                  yz << np.uint64(17) | xz, np.uint64(19) << np.uint64(51) | np.uint64(1) << np.uint64(48))
    frames = np.zeros(n, dtype=A.FRAME_DTYPE)
    frames["offset"] = 100 + 40 * np.arange(n)
    icao = 0x400000 + who
    frames["bytes"][:, 0] = 0x8D
    for k in range(3):
        frames["bytes"][:, 1 + k] = (icao >> (16 - 8 * k)) & 0xFF
    for k in range(7):
        frames["bytes"][:, 4 + k] = (me >> np.uint64(48 - 8 * k)) & np.uint64(0xFF)
    frames["fixed_bit"] = 0xFF
    fixes = np.zeros(n, dtype=A.MLAT_FIX_DTYPE)
    fixes["latitude"], fixes["longitude"], fixes["height_m"] = lat0[who], lon0[who], 9000.0
    fixes["residual_rms_m"], fixes["pdop"], fixes["n_used"] = 5.0, 2.0, 6
    fixes["flags"] = np.where(pos, 0x1 | 0x2 | 0x100, 0x8)
    return frames, fixes


torch.cuda.set_stream(torch.cuda.Stream())  # a stream of our own: a NULL stream would make the ctx create one
stream = torch.cuda.current_stream().cuda_stream
HAVE = hasattr(L.load(), "adsb_track_table_update_mlat")
say(f"==== {args.label}: device {torch.cuda.get_device_name(0)}"
    f"{'' if HAVE else ' (no mlat entry points: update without a reserve only)'}")
dem = A.AdsbDemod(device=0, stream=stream, host_staging=False, max_samples=1 << 16, max_out=1024)
for name, n, n_aircraft in (("a. 64 frames of 8 aircraft", 64, 8), ("b. 32768 frames of 2048 aircraft", 32768, 2048)):
    frames, fixes = make_list(n, n_aircraft, seed=n)
    df = torch.from_numpy(frames.view(np.uint8).reshape(-1)).cuda()
    dx = torch.from_numpy(fixes.view(np.uint8).reshape(-1)).cuda()
    kw = dict(max_aircraft=4096, max_frames=n, seconds_per_sample=0.5e-6)
    with A.TrackTable(dem, **kw) as bare, A.TrackTable(dem, **kw) as table:
        calls = {"update, no reserve": lambda: bare.update_device(df.data_ptr(), n, 0)}
        if HAVE:
            table.mlat_reserve(1000.0)
            calls["update, reserved"] = lambda: table.update_device(df.data_ptr(), n, 0)
            calls["update_mlat"] = lambda: table.update_device(df.data_ptr(), n, 0, mlat_ptr=dx.data_ptr())
        got = {k: [] for k in calls}
        for rep in range(args.warmup + args.reps):       # alternating: one of each per round
            for k, call in calls.items():
                x = timed_ms(call)
                if rep >= args.warmup:
                    got[k].append(x)
        say(f"{name}, frames and fixes in device memory, device time of one update ({args.reps} alternating rounds):")
        for k in calls:
            say(f"  {k:20s} {stats(got[k])}")
        if HAVE:
            m = table.mlat()
            assert len(m) == n_aircraft and int(m["n_checked"].sum()) > 0.5 * n * (args.warmup + args.reps)
            base = np.median(got["update, reserved"])
            say(f"  the merge adds {1e3 * (np.median(got['update_mlat']) - base):.1f} us, "
                f"{1e6 * (np.median(got['update_mlat']) - base) / n:.3f} ns per frame; a reserve alone "
                f"{1e3 * (base - np.median(got['update, no reserve'])):+.1f} us; "
                f"{int(m['n_disagree'].sum())} of {int(m['n_checked'].sum())} checked frames disagree")
    del df, dx
dem.close()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as fh:
        fh.write("\n".join(lines) + "\n")
