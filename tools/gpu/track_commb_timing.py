#!/usr/bin/env python3
"""GPU box helper: what keeping the per-aircraft Comm-B records and settling 5,0 against 6,0
(adsb_track_table_commb_reserve, adsb_track_table_update_commb) costs, measured with device events on the ctx stream
around the update alone, warm, medians of 20 with their range.

Lists of 64 frames of 8 aircraft and of 32 768 frames of 2 048 aircraft, everything in device memory, into tables that
already hold every aircraft (one untimed update first, so no timed update admits anything).  The list is a mix: a third
airborne-velocity squitters (DF17 TC 19 ST 1), the rest DF20 replies of the same aircraft, half of them payloads that
read as 5,0 and as 6,0 and agree with the velocity message, the others BDS 4,0, 1,7 and random MB; one frame in ten
without an aircraft's address.
  a. `update_modes` against `update_commb` of the same build on that list, each on a table of its own, alternating in
     a loop of their own: the difference is what the two scans, the per-frame kernel and the merge add;
  b. plain `update` of a table WITHOUT any reserve on the squitters of that list, and
  c. `update_modes` of a table with the modes reserve only, alternating in a first loop that is the same in every
     build: the figures to hold against the parent commit's library.
The library is whichever ADSB_HIP_LIB names (with ADSB_HIP_LIB_LENIENT=1 for a build without the commb entry points,
e.g. the parent commit's: then only b and c are measured), so passes of two builds can alternate in separate processes.
`--label` names the pass; `--out PATH` appends the report to PATH."""
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
ap.add_argument("--reps", type=int, default=20)
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


def put(mb, first, width, value):
    """MB bits first .. first + width - 1 (numbered from 1) of the (n, 7) byte rows `mb` = value (an array)"""
    for k in range(width):
        bit = first - 1 + k
        on = (value >> (width - 1 - k)) & 1
        mb[:, bit >> 3] = np.where(on == 1, mb[:, bit >> 3] | (0x80 >> (bit & 7)), mb[:, bit >> 3] & ~(0x80 >> (bit & 7)))


def make_list(n, n_aircraft, seed):
    """(frames, modes records, stateless commb records of the CPU mirror) of the mix"""
    rng = np.random.default_rng(seed)
    who = rng.integers(0, n_aircraft, n)
    icao = (0x400000 + who).astype(np.uint32)
    # one state per aircraft: 430 kt towards 254 degrees, level
    frames = np.zeros(n, dtype=A.FRAME_DTYPE)
    frames["offset"] = 100 + 40 * np.arange(n)
    frames["fixed_bit"] = 0xFF
    sort = rng.random(n)
    vel = sort < 1.0 / 3.0
    b = frames["bytes"]
    b[:, 0] = np.where(vel, 0x8D, 20 << 3)
    for k in range(3):
        b[:, 1 + k] = np.where(vel, (icao >> (16 - 8 * k)) & 0xFF, rng.integers(0, 256, n))
    me = np.zeros((n, 7), dtype=np.int64)
    put(me, 1, 5, np.full(n, 19)), put(me, 6, 3, np.full(n, 1))
    put(me, 14, 1, np.full(n, 1)), put(me, 15, 10, np.full(n, 414)), put(me, 25, 1, np.full(n, 1)), put(me, 26, 10, np.full(n, 121))
    put(me, 36, 1, np.full(n, 1)), put(me, 38, 9, np.full(n, 1))
    mb = np.zeros((n, 7), dtype=np.int64)
    kind = rng.integers(0, 6, n)                         # 0-2: 5,0 that reads as 6,0 too; 3: 4,0; 4: 1,7; 5: random
    both = kind <= 2
    put(mb, 1, 1, both | (kind == 3)), put(mb, 2, 10, np.where(both, 0x3DF, rng.integers(0, 1024, n)))
    put(mb, 12, 1, both.astype(np.int64)), put(mb, 13, 11, np.where(both, 0x400 | 420, 0))
    put(mb, 24, 1, both.astype(np.int64)), put(mb, 25, 10, np.where(both, 215, 0))
    put(mb, 35, 1, both.astype(np.int64)), put(mb, 36, 10, np.where(both, 0x3EC, 0))
    put(mb, 46, 1, both.astype(np.int64)), put(mb, 47, 10, np.where(both, 180, 0))
    put(mb, 7, 1, (kind == 4).astype(np.int64)), put(mb, 16, 1, (kind == 4).astype(np.int64))
    rnd = rng.integers(0, 256, size=(n, 7))
    mb = np.where((kind == 5)[:, None], rnd, mb)
    b[:, 4:11] = np.where(vel[:, None], me, mb)
    recs = np.zeros(n, dtype=A.MODES_DTYPE)
    recs["address"], recs["df"] = icao, np.where(vel, 17, 20)
    recs["kind"] = np.where(vel, A.ADSB_MODES_SELF, A.ADSB_MODES_KNOWN)
    lost = ~vel & (rng.random(n) < 0.15)
    recs["kind"][lost] = A.ADSB_MODES_UNKNOWN
    recs["address"][lost] = rng.integers(0, 1 << 24, size=int(lost.sum()))
    return frames, recs, A.host_commb(frames)[0]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()


torch.cuda.set_stream(torch.cuda.Stream())  # a stream of our own: a NULL stream would make the ctx create one
stream = torch.cuda.current_stream().cuda_stream
HAVE = hasattr(L.load(), "adsb_track_table_update_commb")
say(f"==== {args.label}: device {torch.cuda.get_device_name(0)}"
    f"{'' if HAVE else ' (no commb entry points: update and update_modes only)'}")
dem = A.AdsbDemod(device=0, stream=stream, host_staging=False, max_samples=1 << 16, max_out=1024)
for name, n, n_aircraft in (("64 frames of 8 aircraft", 64, 8), ("32768 frames of 2048 aircraft", 32768, 2048)):
    frames, recs, commb = make_list(n, n_aircraft, seed=n)
    squitters = np.ascontiguousarray(frames[recs["df"] == 17])
    df, dr, dc, dsq = dev(frames), dev(recs), dev(commb), dev(squitters)
    kw = dict(max_aircraft=4096, max_frames=n, seconds_per_sample=0.5e-6)
    with A.TrackTable(dem, **kw) as bare, A.TrackTable(dem, **kw) as modes, A.TrackTable(dem, **kw) as table:
        modes.modes_reserve()
        calls = {"b. update, no reserve, squitters": lambda: bare.update_device(dsq.data_ptr(), len(squitters), 0),
                 "c. update_modes, modes reserve": lambda: modes.update_device(df.data_ptr(), n, 0, modes_ptr=dr.data_ptr())}
        if HAVE:
            table.modes_reserve()
            table.commb_reserve()
            calls["a. update_commb, both reserves"] = lambda: table.update_device(df.data_ptr(), n, 0, modes_ptr=dr.data_ptr(),
                                                                                  commb_ptr=dc.data_ptr())
        # two loops, so that b and c run under the same conditions in every build: a third table at work between them
        # (64 MiB of index each) would change what the caches hold when they start
        got = {k: [] for k in calls}
        loops = [[k for k in calls if k[0] in "bc"]] + ([[k for k in calls if k[0] == "c"] + [k for k in calls if k[0] == "a"]] if HAVE else [])
        again = "c. update_modes, beside update_commb"
        if HAVE:
            got[again] = []
        for n_loop, loop in enumerate(loops):
            for rep in range(args.warmup + args.reps):   # alternating: one of each per round
                for k in loop:
                    x = timed_ms(calls[k])
                    if rep >= args.warmup:
                        got[again if n_loop == 1 and k[0] == "c" else k].append(x)
        say(f"{name}, everything in device memory, device time of one update ({args.reps} alternating rounds):")
        for k in got:
            say(f"  {k:38s} {stats(got[k])}")
        if HAVE:
            side, out = table.commb(), table.frame_commb()
            assert len(side) == n_aircraft and int(side["n_settled"].sum()) > 0 and len(out) == n
            add = np.median(got["a. update_commb, both reserves"]) - np.median(got[again])
            say(f"  update_commb adds {1e3 * add:.1f} us to update_modes, {1e6 * add / n:.3f} ns per frame; the list has "
                f"{len(squitters)} velocity squitters, {int((commb['state'] == 4).sum())} ambiguous replies of which "
                f"{int((out['state'] == A.COMMB_SETTLED).sum())} settle, "
                f"{int((recs['kind'] == A.ADSB_MODES_UNKNOWN).sum())} frames without an aircraft")
    del df, dr, dc, dsq
dem.close()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as fh:
        fh.write("\n".join(lines) + "\n")
