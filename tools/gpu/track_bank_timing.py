#!/usr/bin/env python3
"""GPU box helper: cost of one track bank update (adsb_track_bank_update / _update_launch: field decode + sort by
receiver << 24 | icao + hash lookup / per-receiver admission + pairs with record fallback + in-place merge) next to
what the same work costs through per-receiver track tables, measured with device events on the ctx stream.

  1. 64 receivers x one 20 000-sample buffer's list each (1-32 frames per receiver), host frames with a sample_base
     per receiver, from a bank that already holds each receiver's 35 aircraft: device us per bank update over a batch
     of back-to-back updates, and the same lists as 64 TrackTable updates (device us for all 64);
  2. the config-4 workload (64 channels x 8 Mi samples of synthetic i8 in one launch, bench.py --preset config4)
     through update_launch: ms per update into an empty bank and into a bank that already holds every aircraft, next
     to adsb_track_device (field decode + per-launch tracker) on a single-channel list of the same length (one
     512 Mi-sample buffer, the same samples in one channel).
Prints the report; `--out PATH` also writes it to PATH (profiles/track_bank_timing.txt holds a run)."""
import argparse
import contextlib
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

# ---- 1. 64 receivers x one small list each ----------------------------------------------------------------------
R = 64
oracle = Oracle()
pools = []
for r in range(R):
    traffic = random_traffic(oracle, seed=1000 + r, n_aircraft=35, n_frames=600)
    pool = np.zeros(len(traffic), dtype=A.FRAME_DTYPE)
    for k, (_, fr) in enumerate(traffic):
        pool[k]["bytes"] = np.frombuffer(fr, dtype=np.uint8)
        pool[k]["fixed_bit"] = 0xFF
    pools.append(pool)
dem = A.AdsbDemod(device=0, max_samples=1 << 16, max_out=1 << 12, stream=stream, host_staging=False)
say(f"{R} receivers x one 20 000-sample buffer's list (host frames, each receiver holding 35 aircraft):")
say("  frames/receiver  bank us/update  64 tables us (all 64)  ratio  bank wall us/update+points")
sps = 1.0 / 20000
with A.TrackBank(dem, R, max_frames=R * 32, seconds_per_sample=sps) as bank, contextlib.ExitStack() as es:
    tables = [es.enter_context(A.TrackTable(dem, max_frames=32, seconds_per_sample=sps)) for _ in range(R)]
    step = [0]

    def lists(k, u):  # consecutive slices of each receiver's traffic, offsets ascending inside each list
        out = []
        for r in range(R):
            a = (u * k) % (len(pools[r]) - k)
            x = pools[r][a:a + k].copy()
            x["offset"] = 300 + 300 * np.arange(k)
            out.append(x)
        return out

    for k in (1, 8, 16, 32):
        prepared = [lists(k, u) for u in range(16)]
        joined = [np.concatenate(ls) for ls in prepared]
        counts = [k] * R

        def one_bank():
            u = step[0]
            bank.update(joined[u % 16], counts, [20000 * u + 11 * r for r in range(R)])
            step[0] += 1

        def tables_64():
            u = step[0]
            ls = prepared[u % 16]
            for r in range(R):
                tables[r].update(ls[r], sample_base=20000 * u + 11 * r)
            step[0] += 1

        for _ in range(30):
            one_bank()                                      # warm-up (and fills the bank)
            tables_64()
        us_bank = 1e3 * dev_ms(one_bank, 400)
        us_tables = 1e3 * dev_ms(tables_64, 40)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(200):
            one_bank()
            bank.points()
        us_wall = 1e6 * (time.perf_counter() - t0) / 200
        say(f"  {k:15d}  {us_bank:14.2f}  {us_tables:21.2f}  {us_tables / us_bank:5.1f}  {us_wall:26.2f}")
    recs, flags = bank.aircraft()
    say(f"  bank: {sum(len(x) for x in recs)} aircraft in {R} receivers, flags set on {sum(f != 0 for f in flags)}")
dem.close()

# ---- 2. the config-4 workload through update_launch ------------------------------------------------------------
n = 1 << 29
n_ch = (n // R) & ~7
cfg = A.synth_default()
cap = n // cfg.slot_len + 8192
iq = torch.empty(n * 2, dtype=torch.int8, device="cuda")
dem = A.AdsbDemod(device=0, max_samples=n_ch, max_out=cap, max_channels=R, stream=stream, host_staging=False)
for c in range(R):                          # every channel is its own stream (its own generator channel)
    dem.synth_fill_device(cfg, c, 0, n_ch, iq.data_ptr() + c * n_ch * 2)
dem.demod_device_async(iq.data_ptr(), n_ch, n_channels=R, channel_stride=n_ch)
n_out, _, _ = dem.fetch_counts()
say(f"config 4: {n_out} frames from {R} channels x {n_ch} samples in one launch (every synthetic frame has its own ICAO)")
reps = 5
with A.TrackBank(dem, R, max_frames=cap, seconds_per_sample=0.5e-6) as bank:
    for _ in range(2):
        bank.reset()
        bank.update_launch()
    ms_new = []
    for _ in range(reps):
        bank.reset()
        ms_new.append(dev_ms(bank.update_launch, 1))
    say(f"  bank update_launch, empty bank (every ICAO admitted):     {np.mean(ms_new):8.3f} ms "
        f"(min {min(ms_new):.3f}, max {max(ms_new):.3f})")
    base = [0]

    def again():
        base[0] += n_ch
        bank.update_launch([base[0]] * R)

    ms_known = dev_ms(again, reps)
    say(f"  bank update_launch, bank already holds every ICAO:        {ms_known:8.3f} ms")
    recs, flags = bank.aircraft()
    pts = bank.points()
    say(f"  bank: {sum(len(x) for x in recs)} aircraft, {min(len(x) for x in recs)}-{max(len(x) for x in recs)} per "
        f"receiver, flags set on {sum(f != 0 for f in flags)}; last update: {int((pts['flags'] & 1).sum())} new positions")
    frames_dev, _ = dem.result_device()
    _, counts, _, _ = dem.fetch(n_channels=R)

    def from_device():
        base[0] += n_ch
        bank.update_device(frames_dev, n_out, counts, [base[0]] * R)

    ms_split = dev_ms(from_device, reps)
    say(f"  bank update_device, same list, host split (no header sync): {ms_split:8.3f} ms")
    ms_reset = dev_ms(bank.reset, reps)
    say(f"  bank reset (hash {8 * 2 * R * 65536 >> 20} MiB + counters):                    {ms_reset:8.3f} ms")
dem.close()

dem = A.AdsbDemod(device=0, max_samples=n, max_out=cap, stream=stream, host_staging=False)
dem.synth_fill_device(cfg, 0, 0, n, iq.data_ptr())
dem.demod_device_async(iq.data_ptr(), n)
n1, _, _ = dem.fetch_counts()
lib = dem._lib


def track_device():
    assert lib.adsb_decode_fields_device_async(dem.handle) == 0
    assert lib.adsb_track_device(dem.handle, 0.5e-6) == 0


for _ in range(2):
    track_device()
ms_dev = dev_ms(track_device, reps)
say(f"  adsb_track_device, one channel of {n} samples ({n1} frames): {ms_dev:8.3f} ms")
dem.close()

if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
