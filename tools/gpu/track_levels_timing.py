#!/usr/bin/env python3
"""GPU box helper: what the per-aircraft level merge (adsb_track_*_levels_reserve, *_update_levels) costs, measured with
device events on the ctx stream around the update alone, warm, medians with their range.

  a. the benchmark's list (config 4: 64 channels x 8 Mi samples of synthetic i8 in one launch, ~253 k frames, every
     frame its own ICAO), read in device memory, into a FRESH table (a reset before every timed update, outside the
     timed part): every frame admits an aircraft;
  b. 64 receivers x 4 000 frames (35 aircraft per receiver) into a bank that holds them all, frames and levels in
     device memory.
For each: `update` without a levels reserve, `update` with one, and `update_levels`.  The library is whichever
ADSB_HIP_LIB names (with ADSB_HIP_LIB_LENIENT=1 for a build without the levels entry points, e.g. the parent commit's:
then only `update` without a reserve is measured), so one GPU call can alternate builds: "unreserved stores are
unaffected" rests on the parent's figure and this build's first one agreeing within the run-to-run spread the same
report shows.  `--label` names the pass; `--out PATH` appends the report to PATH (a run is meant to be kept as
profiles/track_levels_timing.txt)."""
import argparse
import os
import sys

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
ap.add_argument("--reps", type=int, default=15)
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


torch.cuda.set_stream(torch.cuda.Stream())  # a stream of our own: a NULL stream would make the ctx create one
stream = torch.cuda.current_stream().cuda_stream
HAVE = hasattr(L.load(), "adsb_track_table_levels_reserve")
say(f"==== {args.label}: device {torch.cuda.get_device_name(0)}"
    f"{'' if HAVE else ' (no levels entry points: update without a reserve only)'}")
# (reserve, merge): update without a reserve, update with one, update_levels
variants = [(False, False), (True, False), (True, True)] if HAVE else [(False, False)]
NAMES = {(False, False): "update, no reserve", (True, False): "update, reserved", (True, True): "update_levels"}


def report(got, n):
    for v in variants:
        say(f"  {NAMES[v]:20s} {stats(got[v])}")
    if HAVE:
        base = np.median(got[(False, False)])
        say(f"  the merge adds {1e3 * (np.median(got[(True, True)]) - base):.1f} us, "
            f"{1e6 * (np.median(got[(True, True)]) - base) / n:.3f} ns per frame; a reserve alone "
            f"{1e3 * (np.median(got[(True, False)]) - base):+.1f} us")


# ---- a. the benchmark's list into a fresh table --------------------------------------------------------------------
R, n = 64, 1 << 29
n_ch = (n // R) & ~7
cfg = A.synth_default()
cap = n // cfg.slot_len + 8192
iq = torch.empty(n * 2, dtype=torch.int8, device="cuda")
dem = A.AdsbDemod(device=0, stream=stream, host_staging=False, max_samples=n_ch, max_out=cap, max_channels=R)
for c in range(R):
    dem.synth_fill_device(cfg, c, 0, n_ch, iq.data_ptr() + c * n_ch * 2)
dem.demod_device_async(iq.data_ptr(), n_ch, n_channels=R, channel_stride=n_ch)
n_out, _, _ = dem.fetch_counts()
frames_ptr, _ = dem.result_device()
levels_ptr = None
if HAVE:
    dem.levels_async()
    levels_ptr = dem.levels_device()
got = {}
for reserve, merge in variants:
    with A.TrackTable(dem, max_aircraft=1 << 18, max_frames=cap, seconds_per_sample=0.5e-6) as t:
        if reserve:
            t.levels_reserve()

        def one():
            if merge:
                t.update_device(frames_ptr, n_out, 0, levels_ptr=levels_ptr)
            else:
                t.update_device(frames_ptr, n_out, 0)

        ms = []
        for k in range(2 + args.reps):
            t.reset()
            x = timed_ms(one)
            if k >= 2:
                ms.append(x)
        got[(reserve, merge)] = ms
        assert len(t.aircraft()[0]) > 0.9 * n_out
say(f"a. config 4's list ({n_out} frames in device memory) into a fresh table, device time of the update:")
report(got, n_out)
dem.close()
del iq

# ---- b. 64 receivers x 4000 frames into a bank ------------------------------------------------------------------------
oracle = Oracle()
K = 4000
parts = []
for r in range(R):
    traffic = random_traffic(oracle, seed=2000 + r, n_aircraft=35, n_frames=K)
    x = np.zeros(K, dtype=A.FRAME_DTYPE)
    x["bytes"] = np.array([np.frombuffer(fr, dtype=np.uint8) for _, fr in traffic])
    x["offset"] = 300 + 300 * np.arange(K)
    x["fixed_bit"] = 0xFF
    parts.append(x)
frames = np.concatenate(parts)
rng = np.random.default_rng(7)
lv = np.zeros(len(frames), dtype=A.LEVEL_DTYPE)
lv["signal_sum"] = rng.integers(0, 1 << 38, size=len(lv), dtype=np.uint64)
lv["noise_sum"] = rng.integers(0, 1 << 38, size=len(lv), dtype=np.uint64)
lv["peak"] = rng.integers(0, 1 << 31, size=len(lv))
lv["weak_bits"] = rng.integers(0, 113, size=len(lv))
lv["flags"] = (rng.random(len(lv)) >= 0.2).astype(np.uint16)
dev_frames = torch.from_numpy(frames.view(np.uint8).copy()).cuda()
dev_levels = torch.from_numpy(lv.view(np.uint8).copy()).cuda()
dem = A.AdsbDemod(device=0, stream=stream, host_staging=False, max_samples=1 << 16, max_out=1 << 12)
got = {}
for reserve, merge in variants:
    with A.TrackBank(dem, R, max_aircraft=64, max_frames=R * K, seconds_per_sample=1.0 / 20000) as b:
        if reserve:
            b.levels_reserve()
        step = [0]

        def one():
            step[0] += 1
            bases = [300 * K * step[0] + 11 * r for r in range(R)]
            if merge:
                b.update_device(dev_frames.data_ptr(), R * K, [K] * R, bases, levels_ptr=dev_levels.data_ptr())
            else:
                b.update_device(dev_frames.data_ptr(), R * K, [K] * R, bases)

        for _ in range(2):
            one()                           # the bank now holds every aircraft
        got[(reserve, merge)] = [timed_ms(one) for _ in range(args.reps)]
say(f"b. {R} receivers x {K} frames (device memory, 35 aircraft per receiver) into a bank that holds them all:")
report(got, R * K)
dem.close()

if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as fh:
        fh.write("\n".join(lines) + "\n")
