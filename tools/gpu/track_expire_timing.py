#!/usr/bin/env python3
"""GPU box helper: cost of expiring stale aircraft (adsb_track_table_expire / adsb_track_bank_expire: mark + rocPRIM scan
+ in-place compaction, plus for a bank the hash clear and reinsertion), measured with device events on the ctx stream.

  1. a full table (65 536 aircraft), evicting 0 %, 10 % and 100 % of them: device us per expire (the table is refilled
     between expires, outside the timed region);
  2. a full bank of 64 receivers x 65 536 aircraft with the same shares;
  3. one small update (8 frames, a table holding 35 aircraft) right after an expire, against one without: device us
     of the update alone, to show that an expire leaves no lasting cost.
Prints the report; `--out PATH` also writes it to PATH (profiles/track_expire_timing.txt holds a run)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import air_rs_amd as A

ap = argparse.ArgumentParser()
ap.add_argument("--out", help="also write the report to this file")
ap.add_argument("--reps", type=int, default=10)
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


def ident_frames(icaos):
    """identification frames (TC 4) of the given ICAOs, one each, offsets 0, 1, 2, ... (the tracker reads the fields
    only; the CRC is not looked at)"""
    f = np.zeros(len(icaos), dtype=A.FRAME_DTYPE)
    b = np.zeros((len(icaos), 14), dtype=np.uint8)
    b[:, 0] = 0x8D
    b[:, 1], b[:, 2], b[:, 3] = (icaos >> 16) & 0xFF, (icaos >> 8) & 0xFF, icaos & 0xFF
    b[:, 4] = 4 << 3
    b[:, 5:11] = 0x41
    f["bytes"] = b
    f["offset"] = np.arange(len(icaos))
    f["fixed_bit"] = 0xFF
    return f


def stats(xs):
    return f"{1e3 * np.median(xs):9.1f} us (min {1e3 * min(xs):.1f}, max {1e3 * max(xs):.1f})"


torch.cuda.set_stream(torch.cuda.Stream())  # a stream of our own: a NULL stream would make the ctx create one
stream = torch.cuda.current_stream().cuda_stream
say(f"device {torch.cuda.get_device_name(0)}")
rng = np.random.default_rng(1)
M, R, sps = 65536, 64, 1e-3
icaos = rng.choice(np.arange(1, 1 << 24), size=M, replace=False).astype(np.uint32)  # list order unrelated to ICAO
full = ident_frames(icaos)
shares = (0.0, 0.1, 1.0)

# ---- 1. a full table ----------------------------------------------------------------------------------------------
dem = A.AdsbDemod(device=0, max_samples=1 << 16, max_out=1 << 12, stream=stream, host_staging=False)
say(f"table, full ({M} aircraft), per expire:")
with A.TrackTable(dem, max_aircraft=M, max_frames=M, seconds_per_sample=sps) as t:
    base = 0
    for share in shares:
        ms = []
        for rep in range(args.reps + 2):
            base += 2 * M                                  # every aircraft heard again, frame k at base + k
            t.update(full, base)
            ms.append(timed_ms(lambda: t.expire((base + share * M) * sps)))
            if rep == 0:
                recs, flags = t.aircraft()
                assert len(recs) == M - round(share * M) and flags == 0, (len(recs), share)
        say(f"  evicting {100 * share:5.1f} %: {stats(ms[2:])}")
dem.close()

# ---- 2. a full bank -----------------------------------------------------------------------------------------------
lists = np.concatenate([full] * R)
dem = A.AdsbDemod(device=0, max_samples=1 << 16, max_out=1 << 12, stream=stream, host_staging=False)
say(f"bank, {R} receivers x {M} aircraft, full, per expire:")
with A.TrackBank(dem, R, max_aircraft=M, max_frames=R * M, seconds_per_sample=sps) as bank:
    base = 0
    for share in shares:
        ms = []
        for rep in range(max(args.reps // 2, 3) + 1):
            base += 2 * M
            bank.update(lists, [M] * R, base)
            ms.append(timed_ms(lambda: bank.expire((base + share * M) * sps)))
            if rep == 0:
                recs, _ = bank.aircraft()
                assert all(len(x) == M - round(share * M) for x in recs), share
        say(f"  evicting {100 * share:5.1f} %: {stats(ms[1:])}")
dem.close()

# ---- 3. a small update after an expire ----------------------------------------------------------------------------
dem = A.AdsbDemod(device=0, max_samples=1 << 16, max_out=1 << 12, stream=stream, host_staging=False)
say("small update (8 frames; a table holding 35 aircraft, max_aircraft 65536), device time of the update alone:")
few = ident_frames(icaos[:35])
with A.TrackTable(dem, max_frames=64, seconds_per_sample=sps) as t:
    t.update(few, 0)
    for label, pre in (("without an expire before it", None), ("right after an expire       ", -1.0)):
        ms = []
        for rep in range(200):
            if pre is not None:
                t.expire(pre)                              # evicts nothing: the table stays at 35
            ms.append(timed_ms(lambda: t.update(few[rep % 4 * 8:rep % 4 * 8 + 8], 100 * rep)))
        say(f"  {label}: {stats(ms[20:])}")
    ms = [timed_ms(lambda: t.expire(-1.0)) for _ in range(50)]
    say(f"  the expire itself (35 aircraft):  {stats(ms[5:])}")
dem.close()

if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
