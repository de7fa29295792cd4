#!/usr/bin/env python3
"""GPU box helper: what positions from single messages (adsb_track_*_fixes_reserve) cost an update, measured with
device events on the ctx stream around the update alone, warm, medians with their range.

One list of 65 536 frames (2 000 aircraft around one site: surface and airborne position messages, velocity,
identification and other type codes; tests/fix_model.mixed_traffic) in device memory, into a table that already holds
every aircraft: `update` without a fixes reserve, and `update` with one.  The library is whichever ADSB_HIP_LIB names
(with ADSB_HIP_LIB_LENIENT=1 for a build without the fixes entry points, e.g. the parent commit's: then only the update
without a reserve is measured), so one GPU call can alternate builds: "a store without the reserve is unaffected" rests
on the parent's figure and this build's first one agreeing within the run-to-run spread the same report shows.
`--label` names the pass; `--out PATH` appends the report to PATH (a run is meant to be kept as
profiles/track_fixes_timing.txt)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import air_rs_amd as A
from air_rs_amd import _lib as L
from tests import fix_model as M
from tests.oracle_binding import Oracle

ap = argparse.ArgumentParser()
ap.add_argument("--out", help="append the report to this file")
ap.add_argument("--label", default="this build")
ap.add_argument("--reps", type=int, default=25)
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
HAVE = hasattr(L.load(), "adsb_track_table_fixes_reserve")
say(f"==== {args.label}: device {torch.cuda.get_device_name(0)}"
    f"{'' if HAVE else ' (no fixes entry points: update without a reserve only)'}")

N, SITE = 1 << 16, (47.45, 8.56, 150.0)
frames = M.mixed_traffic(Oracle(), seed=3, site=SITE, n_aircraft=2000, n_frames=N, span_s=600.0).astype(A.FRAME_DTYPE)
dev_frames = torch.from_numpy(frames.view(np.uint8).copy()).cuda()
dem = A.AdsbDemod(device=0, stream=stream, host_staging=False, max_samples=1 << 16, max_out=1 << 12)
got = {}
for reserve in ([False, True] if HAVE else [False]):
    with A.TrackTable(dem, max_aircraft=4096, max_frames=N, seconds_per_sample=0.5e-6) as t:
        if reserve:
            t.fixes_reserve(SITE)
        step = [0]

        def one():
            step[0] += 1
            t.update_device(dev_frames.data_ptr(), N, 1_200_000_000 * step[0])

        for _ in range(3):
            one()                           # the table now holds every aircraft
        got[reserve] = [timed_ms(one) for _ in range(args.reps)]
        assert len(t.aircraft()[0]) == 2000
        if reserve:
            fx = t.fixes()
            say(f"  ({int((fx['n_fixes'] > 0).sum())} of {len(fx)} aircraft have a fix, "
                f"{int(fx['n_rejected'].sum()) // step[0]} of the list's position messages are turned away)")
say(f"{N} frames (device memory, 2000 aircraft) into a table that holds them all, device time of the update:")
say(f"  update, no reserve   {stats(got[False])}")
if HAVE:
    base = np.median(got[False])
    say(f"  update, reserved     {stats(got[True])}")
    say(f"  the fixes add {1e3 * (np.median(got[True]) - base):.1f} us, "
        f"{1e6 * (np.median(got[True]) - base) / N:.3f} ns per frame")
dem.close()

if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as fh:
        fh.write("\n".join(lines) + "\n")
