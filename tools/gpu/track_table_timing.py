#!/usr/bin/env python3
"""GPU box helper: cost of one persistent track table update (adsb_track_table_update: field decode + sort +
lookup/admission + pairs with table fallback + in-place merge), measured with device events on the ctx stream.

  1. small lists, what one 20 000-sample buffer yields (0-64 frames), host frames with sample_base, from a table
     that already holds the 35 aircraft of tests.traffic's synthetic traffic: device us per update over a batch
     of back-to-back updates, and host wall us per update + points fetch (the latency a caller sees);
  2. the frame list of the bench workload (1 GiB synthetic i8 buffer, ~253 k frames, one ICAO per frame) from
     device memory: ms per update into an empty table and into a table that already holds every ICAO, next to
     adsb_track_device (field decode + per-launch tracker) on the same list.
Prints the report; `--out PATH` also writes it to PATH (profiles/track_table_timing.txt holds a run)."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import air_rs_amd as A
from tests.oracle_binding import Oracle
from tests.traffic import random_traffic

ap = argparse.ArgumentParser()
ap.add_argument("--out", help="also write the report to this file")
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


torch.cuda.set_stream(torch.cuda.Stream())  # a stream of our own: a NULL stream would make the ctx create one
stream = torch.cuda.current_stream().cuda_stream
say(f"device {torch.cuda.get_device_name(0)}")

# ---- 1. small lists --------------------------------------------------------------------------------------------
traffic = random_traffic(Oracle(), seed=21, n_aircraft=35, n_frames=3000)
pool = np.zeros(len(traffic), dtype=A.FRAME_DTYPE)
for k, (_, fr) in enumerate(traffic):
    pool[k]["bytes"] = np.frombuffer(fr, dtype=np.uint8)
    pool[k]["fixed_bit"] = 0xFF
dem = A.AdsbDemod(device=0, max_samples=1 << 16, max_out=1 << 12, stream=stream, host_staging=False)
say("small lists (one 20 000-sample buffer's list, host frames, table holding 35 aircraft):")
say("  frames  device us/update  wall us/update+points")
with A.TrackTable(dem, max_frames=64, seconds_per_sample=1.0 / 20000) as t:
    pos = [0, 0]

    def lists(k):  # consecutive slices of the traffic, offsets ascending inside each list
        out = []
        for a in range(0, len(pool) - 64, max(k, 1)):
            x = pool[a:a + k].copy()
            x["offset"] = 300 + 300 * np.arange(k)
            out.append(x)
        return out

    for k in (0, 1, 8, 16, 32, 64):
        ls = lists(k)

        def one():
            t.update(ls[pos[0] % len(ls)], sample_base=20000 * pos[1])
            pos[0] += 1
            pos[1] += 1

        for _ in range(50):
            one()                                           # warm-up (and fills the table)
        us_dev = 1e3 * dev_ms(one, 2000)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(500):
            one()
            t.points()
        us_wall = 1e6 * (time.perf_counter() - t0) / 500
        say(f"  {k:6d}  {us_dev:16.2f}  {us_wall:21.2f}")
    recs, flags = t.aircraft()
    say(f"  table: {len(recs)} aircraft, flags {flags}")
dem.close()

# ---- 2. the bench buffer's list ----------------------------------------------------------------------------------
n = 1 << 29
cfg = A.synth_default()
cap = n // cfg.slot_len + 8192
dem = A.AdsbDemod(device=0, max_samples=n, max_out=cap, stream=stream, host_staging=False)
iq = torch.empty(n * 2, dtype=torch.int8, device="cuda")
dem.synth_fill_device(cfg, 0, 0, n, iq.data_ptr())
dem.demod_device_async(iq.data_ptr(), n)
n_out, _, _ = dem.fetch_counts()
frames_dev, _ = dem.result_device()
lib = dem._lib
say(f"bench list: {n_out} frames from a 1 GiB i8 buffer (every synthetic frame has its own ICAO)")
reps = 5


def track_device():
    assert lib.adsb_decode_fields_device_async(dem.handle) == 0
    assert lib.adsb_track_device(dem.handle, 0.5e-6) == 0


for _ in range(2):
    track_device()
ms_dev = dev_ms(track_device, reps)
say(f"  adsb_track_device (field decode + tracker, empty map):     {ms_dev:8.3f} ms")
with A.TrackTable(dem, max_aircraft=1 << 19, max_frames=cap, seconds_per_sample=0.5e-6) as t:
    for _ in range(2):
        t.reset()
        t.update_device(frames_dev, n_out)
    ms_new = []
    for _ in range(reps):
        t.reset()
        ms_new.append(dev_ms(lambda: t.update_device(frames_dev, n_out), 1))
    say(f"  table update, empty table (every ICAO admitted):          {np.mean(ms_new):8.3f} ms "
        f"(min {min(ms_new):.3f}, max {max(ms_new):.3f})")
    base = [0]

    def again():
        base[0] += n
        t.update_device(frames_dev, n_out, sample_base=base[0])

    ms_known = dev_ms(again, reps)
    say(f"  table update, table already holds every ICAO:             {ms_known:8.3f} ms")
    recs, flags = t.aircraft()
    pts = t.points()
    say(f"  table: {len(recs)} aircraft, flags {flags}; last update: {int((pts['flags'] & 1).sum())} new positions")
    ms_reset = dev_ms(t.reset, reps)
    say(f"  table reset (64 MiB index + counters):                    {ms_reset:8.3f} ms")

if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
