#!/usr/bin/env python3
"""GPU box helper: what keying a table update by the Mode S stage's addresses and keeping the per-aircraft modes records
(adsb_track_table_modes_reserve, adsb_track_table_update_modes) costs, measured with device events on the ctx stream
around the update alone, warm, medians of 20 with their range.

Lists of 64 and of 32 768 frames, everything in device memory, into tables that already hold every aircraft (one untimed
update first, so no timed update admits anything):
  a. a squitter-only list (every frame a SELF DF17): `update_mlat` against `update_modes` with the same fixes.  The
     difference is what the key kernel, the 25th sort bit, the per-frame kernel, the scan and the merge add;
  b. a realistic mix, about a third SELF squitters, the rest DF4/5/11/20 replies of known aircraft and one frame in ten
     without an aircraft's address: `update_modes` with fixes, and `update_mlat` on the squitters alone for scale;
  c. plain `update` of a table WITHOUT any reserve on list a: the figure to hold against the parent commit's library.
The library is whichever ADSB_HIP_LIB names (with ADSB_HIP_LIB_LENIENT=1 for a build without the modes entry points,
e.g. the parent commit's: then only c is measured), so passes of two builds can alternate in separate processes.
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


def make_lists(n, n_aircraft, seed):
    """(squitter-only frames, their records), (mixed frames, their records), fixes for n frames.  Records are written
    directly: SELF for a squitter, KNOWN for a reply, UNKNOWN for one frame in ten of the mix."""
    rng = np.random.default_rng(seed)
    who = rng.integers(0, n_aircraft, n)
    icao = (0x400000 + who).astype(np.uint32)
    frames = np.zeros(n, dtype=A.FRAME_DTYPE)
    frames["offset"] = 100 + 40 * np.arange(n)
    frames["bytes"][:, 0] = 0x8D
    for k in range(3):
        frames["bytes"][:, 1 + k] = (icao >> (16 - 8 * k)) & 0xFF
    frames["bytes"][:, 4] = np.where(rng.random(n) < 0.5, 19 << 3 | 1, 4 << 3)      # velocity and identification messages
    frames["bytes"][:, 5:11] = rng.integers(0, 256, size=(n, 6))
    frames["fixed_bit"] = 0xFF
    recs = np.zeros(n, dtype=A.MODES_DTYPE)
    recs["address"], recs["df"], recs["kind"] = icao, 17, A.ADSB_MODES_SELF
    mixed, mrecs = frames.copy(), recs.copy()
    sort = rng.random(n)
    reply = sort >= 1.0 / 3.0
    df = rng.choice([4, 5, 11, 20], size=n).astype(np.uint8)
    mixed["bytes"][reply, 0] = df[reply] << 3
    mixed["bytes"][reply, 1:4] = rng.integers(0, 256, size=(int(reply.sum()), 3))   # FS/DR/UM/AC, not the address
    mrecs["df"][reply] = df[reply]
    mrecs["kind"][reply] = A.ADSB_MODES_KNOWN
    mrecs["flags"][reply & (df == 4)] = A.ADSB_MODES_ALT
    mrecs["flags"][reply & (df == 5)] = A.ADSB_MODES_SQUAWK
    mrecs["flags"][reply & (df == 20)] = A.ADSB_MODES_ALT | A.ADSB_MODES_CALLSIGN
    mrecs["altitude_ft"], mrecs["squawk"], mrecs["callsign"] = 30000, 4210, b"TIMING1_"
    lost = sort >= 0.9
    mrecs["kind"][lost] = A.ADSB_MODES_UNKNOWN
    mrecs["address"][lost] = rng.integers(0, 1 << 24, size=int(lost.sum()))
    fixes = np.zeros(n, dtype=A.MLAT_FIX_DTYPE)
    fixes["latitude"], fixes["longitude"], fixes["height_m"] = 47.0, 8.0, 9000.0
    fixes["residual_rms_m"], fixes["pdop"], fixes["n_used"] = 5.0, 2.0, 6
    fixes["flags"] = A.ADSB_MLAT_ATTEMPTED | A.ADSB_MLAT_CONVERGED | A.ADSB_MLAT_VALID
    return (frames, recs), (mixed, mrecs), fixes


def dev(a):
    return torch.from_numpy(a.view(np.uint8).reshape(-1)).cuda()


torch.cuda.set_stream(torch.cuda.Stream())  # a stream of our own: a NULL stream would make the ctx create one
stream = torch.cuda.current_stream().cuda_stream
HAVE = hasattr(L.load(), "adsb_track_table_update_modes")
say(f"==== {args.label}: device {torch.cuda.get_device_name(0)}"
    f"{'' if HAVE else ' (no modes entry points: update without a reserve only)'}")
dem = A.AdsbDemod(device=0, stream=stream, host_staging=False, max_samples=1 << 16, max_out=1024)
for name, n, n_aircraft in (("64 frames of 8 aircraft", 64, 8), ("32768 frames of 2048 aircraft", 32768, 2048)):
    (frames, recs), (mixed, mrecs), fixes = make_lists(n, n_aircraft, seed=n)
    squitters = np.ascontiguousarray(mixed[mrecs["df"] == 17])
    df, dr, dm, dmr, dx, dsq = dev(frames), dev(recs), dev(mixed), dev(mrecs), dev(fixes), dev(squitters)
    kw = dict(max_aircraft=4096, max_frames=n, seconds_per_sample=0.5e-6)
    with A.TrackTable(dem, **kw) as bare, A.TrackTable(dem, **kw) as table, A.TrackTable(dem, **kw) as mix:
        calls = {"c. update, no reserve": lambda: bare.update_device(df.data_ptr(), n, 0)}
        if HAVE:
            for t in (table, mix):
                t.mlat_reserve(1000.0)
                t.modes_reserve()
            calls["a. update_mlat, squitters"] = lambda: table.update_device(df.data_ptr(), n, 0, mlat_ptr=dx.data_ptr())
            calls["a. update_modes, squitters"] = lambda: table.update_device(df.data_ptr(), n, 0, mlat_ptr=dx.data_ptr(),
                                                                              modes_ptr=dr.data_ptr())
            calls["b. update_modes, mix"] = lambda: mix.update_device(dm.data_ptr(), n, 0, mlat_ptr=dx.data_ptr(),
                                                                      modes_ptr=dmr.data_ptr())
            calls["b. update_mlat, its squitters"] = lambda: mix.update_device(dsq.data_ptr(), len(squitters), 0,
                                                                               mlat_ptr=dx.data_ptr())
        got = {k: [] for k in calls}
        for rep in range(args.warmup + args.reps):       # alternating: one of each per round
            for k, call in calls.items():
                x = timed_ms(call)
                if rep >= args.warmup:
                    got[k].append(x)
        say(f"{name}, everything in device memory, device time of one update ({args.reps} alternating rounds):")
        for k in calls:
            say(f"  {k:32s} {stats(got[k])}")
        if HAVE:
            side = mix.modes()
            assert len(side) == n_aircraft and int(side["n_replies"].sum()) > 0
            add = np.median(got["a. update_modes, squitters"]) - np.median(got["a. update_mlat, squitters"])
            say(f"  on squitters update_modes adds {1e3 * add:.1f} us to update_mlat, {1e6 * add / n:.3f} ns per frame; "
                f"the mix has {len(squitters)} squitters, {int((mrecs['kind'] == A.ADSB_MODES_KNOWN).sum())} replies, "
                f"{int((mrecs['kind'] == A.ADSB_MODES_UNKNOWN).sum())} frames without an aircraft")
    del df, dr, dm, dmr, dx, dsq
dem.close()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as fh:
        fh.write("\n".join(lines) + "\n")
