#!/usr/bin/env python3
"""GPU box helper: cost of track table and bank updates on traffic where about a third of the frames are airborne-
velocity messages (DF17 TC 19, tests.velocity_traffic), measured with device events on the ctx stream.  Runs against
any build of the library (ADSB_HIP_LIB, with ADSB_HIP_LIB_LENIENT=1 for one without the velocity entry points), so
the same traffic times a build that decodes velocity and one that does not.

  1. small table updates: lists of 1-32 host frames (what one 20 000-sample buffer yields) into a table that already
     holds the traffic's 35 aircraft: device us per update over a batch of back-to-back updates;
  2. a 64-receiver bank update of 16 frames per receiver, each receiver holding 35 aircraft: device us per update.
Prints the report; `--out PATH` also writes it to PATH (profiles/track_velocity_timing.txt holds runs)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import air_rs_amd as A
from air_rs_amd import _lib
from tests.oracle_binding import Oracle
from tests.velocity_traffic import velocity_traffic

ap = argparse.ArgumentParser()
ap.add_argument("--out", help="also write the report to this file")
ap.add_argument("--label", default="", help="a name for the library under test, printed in the report")
args = ap.parse_args()
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def dev_ms(fn, reps):
    st = torch.cuda.current_stream()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record(st)
    for _ in range(reps):
        fn()
    b.record(st)
    b.synchronize()
    return a.elapsed_time(b) / reps


def pool(oracle, seed):
    traffic = velocity_traffic(oracle, seed=seed, n_aircraft=35, n_frames=600)
    out = np.zeros(len(traffic), dtype=A.FRAME_DTYPE)
    for k, (_, fr) in enumerate(traffic):
        out[k]["bytes"] = np.frombuffer(fr, dtype=np.uint8)
        out[k]["fixed_bit"] = 0xFF
    return out


def lists(p, k, n):  # n consecutive slices of k frames, offsets ascending inside each list
    out = []
    for u in range(n):
        a = (u * k) % (len(p) - k)
        x = p[a:a + k].copy()
        x["offset"] = 300 + 300 * np.arange(k)
        out.append(x)
    return out


torch.cuda.set_stream(torch.cuda.Stream())  # a stream of our own: a NULL stream would make the ctx create one
stream = torch.cuda.current_stream().cuda_stream
has_velocity = hasattr(_lib.load(), "adsb_track_table_fetch_velocity")
say(f"device {torch.cuda.get_device_name(0)}; library {args.label or _lib.LIB_PATH} "
    f"({'decodes' if has_velocity else 'does not decode'} velocity)")
oracle = Oracle()
pools = [pool(oracle, 2000 + r) for r in range(64)]
tc19 = np.mean([(p["bytes"][:, 4] >> 3 == 19).mean() for p in pools])
say(f"traffic: {100 * tc19:.0f} % of the frames are TC 19")
dem = A.AdsbDemod(device=0, max_samples=1 << 16, max_out=1 << 12, stream=stream, host_staging=False)
sps = 1.0 / 20000
step = [0]

say("1. small table updates (table holding 35 aircraft):")
say("  frames/update  device us/update")
with A.TrackTable(dem, max_frames=64, seconds_per_sample=sps) as t:
    for k in (1, 8, 16, 32):
        prepared = lists(pools[0], k, 16)

        def one():
            u = step[0]
            t.update(prepared[u % 16], sample_base=20000 * u)
            step[0] += 1

        for _ in range(30):
            one()
        say(f"  {k:13d}  {1e3 * dev_ms(one, 400):16.2f}")
    if has_velocity:
        vel = t.velocity()
        say(f"  table: {len(vel)} aircraft, {int((vel['subtype'] != 0).sum())} with a velocity")

R, k = 64, 16
say(f"2. {R}-receiver bank update, {k} frames per receiver (each receiver holding 35 aircraft):")
with A.TrackBank(dem, R, max_frames=R * k, seconds_per_sample=sps) as bank:
    prepared = [lists(pools[r], k, 16) for r in range(R)]
    joined = [np.concatenate([prepared[r][u] for r in range(R)]) for u in range(16)]

    def one_bank():
        u = step[0]
        bank.update(joined[u % 16], [k] * R, [20000 * u + 11 * r for r in range(R)])
        step[0] += 1

    for _ in range(30):
        one_bank()
    say(f"  device us/update: {1e3 * dev_ms(one_bank, 400):.2f}")
dem.close()

if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
