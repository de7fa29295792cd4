#!/usr/bin/env python3
"""GPU box helper: what keeping the per-aircraft extended squitter records and resolving NIC and Rc
(adsb_track_table_es_reserve, adsb_track_table_update_es) costs, measured with device events on the ctx stream around
the update alone, warm, medians of 20 with their range.

Lists of 64 frames of 8 aircraft and of 32 768 frames of 2 048 aircraft, everything in device memory, into tables that
already hold every aircraft (the five warm-up rounds come first, so no timed update admits anything).  The list is a mix: two
thirds DF17 extended squitters (positions of every type code, operational status of versions 0-2 airborne and surface,
target state, TC 28, velocities, identifications), a third DF20 replies of the same aircraft with random MB; one reply
in seven without an aircraft's address.
  a. what update_es adds to the update it extends, each pair on tables of their own, alternating in a loop of their own:
     plain `update` against `update_es` on the squitters of the list, `update_modes` against `update_es` with the modes
     records on the whole list, and beside them `update_commb` against the same `update_modes`: the Comm-B step's added
     cost from the same run, as the reference point;
  b. plain `update` of a table WITHOUT any reserve on the squitters of that list, and
  c. `update_modes` of a table with the modes reserve only, alternating in a first loop that is the same in every
     build and runs before anything that is not (the other tables' reserves, the stateless records): the figures to
     hold against the parent commit's library.
The library is whichever ADSB_HIP_LIB names (with ADSB_HIP_LIB_LENIENT=1 for a build without the es entry points, e.g.
the parent commit's: then only b and c are measured), so passes of two builds can alternate in separate processes.
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


def make_list(n, n_aircraft, seed):
    """(frames, modes records) of the mix; the stateless es and commb records come from the CPU mirrors"""
    rng = np.random.default_rng(seed)
    icao = (0x400000 + rng.integers(0, n_aircraft, n)).astype(np.uint32)
    frames = np.zeros(n, dtype=A.FRAME_DTYPE)
    frames["offset"] = 100 + 40 * np.arange(n)
    frames["fixed_bit"] = 0xFF
    squitter = rng.random(n) < 2.0 / 3.0
    b = frames["bytes"]
    b[:, 4:11] = rng.integers(0, 256, size=(n, 7))
    b[:, 0] = np.where(squitter, 0x8D, 20 << 3)
    for k in range(3):
        b[:, 1 + k] = np.where(squitter, (icao >> (16 - 8 * k)) & 0xFF, rng.integers(0, 256, n))
    # ME byte 0: a type code and subtype of the kinds the stage reads; the operational status's version in bytes[9] bits 7-5
    sort = rng.integers(0, 8, n)
    tc = np.select([sort < 3, sort == 3, sort == 4, sort == 5, sort == 6], [rng.integers(5, 19, n), 31, 29, 28, 19], rng.integers(1, 5, n))
    st = np.select([tc == 31, tc == 29, tc == 28, tc == 19], [rng.integers(0, 2, n), 2 | rng.integers(0, 2, n), rng.integers(1, 3, n), 1],
                   rng.integers(0, 8, n))
    b[:, 4] = np.where(squitter, tc << 3 | st, b[:, 4])
    b[:, 9] = np.where(squitter & (tc == 31), (b[:, 9] & 0x1F) | rng.integers(0, 3, n) << 5, b[:, 9])
    recs = np.zeros(n, dtype=A.MODES_DTYPE)
    recs["address"], recs["df"] = icao, np.where(squitter, 17, 20)
    recs["kind"] = np.where(squitter, A.ADSB_MODES_SELF, A.ADSB_MODES_KNOWN)
    lost = ~squitter & (rng.random(n) < 1.0 / 7.0)
    recs["kind"][lost] = A.ADSB_MODES_UNKNOWN
    recs["address"][lost] = rng.integers(0, 1 << 24, size=int(lost.sum()))
    return frames, recs


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()


torch.cuda.set_stream(torch.cuda.Stream())  # a stream of our own: a NULL stream would make the ctx create one
stream = torch.cuda.current_stream().cuda_stream
HAVE = hasattr(L.load(), "adsb_track_table_update_es")
say(f"==== {args.label}: device {torch.cuda.get_device_name(0)}"
    f"{'' if HAVE else ' (no es entry points: update and update_modes only)'}")
dem = A.AdsbDemod(device=0, stream=stream, host_staging=False, max_samples=1 << 16, max_out=1024)
for name, n, n_aircraft in (("64 frames of 8 aircraft", 64, 8), ("32768 frames of 2048 aircraft", 32768, 2048)):
    frames, recs = make_list(n, n_aircraft, seed=n)
    is_squitter = recs["df"] == 17
    squitters = np.ascontiguousarray(frames[is_squitter])
    df, dr, dsq = dev(frames), dev(recs), dev(squitters)
    kw = dict(max_aircraft=4096, max_frames=n, seconds_per_sample=0.5e-6)
    tables = [A.TrackTable(dem, **kw) for _ in range(6)]
    bare, modes, plain, plain_es, keyed_es, commb_t = tables
    modes.modes_reserve()
    calls = {"b. update, no reserve, squitters": lambda: bare.update_device(dsq.data_ptr(), len(squitters), 0),
             "c. update_modes, modes reserve": lambda: modes.update_device(df.data_ptr(), n, 0, modes_ptr=dr.data_ptr())}
    got = {}

    def run(loop):
        for k in loop:
            got[k] = []
        for rep in range(args.warmup + args.reps):       # alternating: one of each per round
            for k in loop:
                x = timed_ms(calls[k])
                if rep >= args.warmup:
                    got[k].append(x)

    # b and c first, before this build does anything the parent's cannot: the reserves of the other tables, their
    # clears and pinned allocations, and the stateless records all come after this loop, so that it runs under the
    # same conditions in every build
    run(list(calls))
    if HAVE:
        es = A.host_es(frames)[0]
        commb = A.host_commb(frames)[0]
        de, desq, dc = dev(es), dev(np.ascontiguousarray(es[is_squitter])), dev(commb)
        plain_es.es_reserve()
        keyed_es.modes_reserve(), keyed_es.es_reserve()
        commb_t.modes_reserve(), commb_t.commb_reserve()
        more = {"a1. update, squitters": lambda: plain.update_device(dsq.data_ptr(), len(squitters), 0),
                "a2. update_es, squitters": lambda: plain_es.update_device(dsq.data_ptr(), len(squitters), 0, es_ptr=desq.data_ptr()),
                "a3. update_modes": lambda: modes.update_device(df.data_ptr(), n, 0, modes_ptr=dr.data_ptr()),
                "a4. update_es with modes": lambda: keyed_es.update_device(df.data_ptr(), n, 0, modes_ptr=dr.data_ptr(), es_ptr=de.data_ptr()),
                "a5. update_commb": lambda: commb_t.update_device(df.data_ptr(), n, 0, modes_ptr=dr.data_ptr(), commb_ptr=dc.data_ptr())}
        calls.update(more)
        run(list(more))
    say(f"{name}, everything in device memory, device time of one update ({args.reps} alternating rounds):")
    for k in got:
        say(f"  {k:38s} {stats(got[k])}")
    if HAVE:
        side, out = keyed_es.es(), keyed_es.frame_es()
        assert len(side) == n_aircraft and int(side["n_position"].sum()) > 0 and len(out) == n
        if len(plain_es.es()) == len(side):                                # both paths count the same squitters
            assert plain_es.es().tobytes() == side.tobytes()
        med = lambda k: float(np.median(got[k]))
        add_plain, add_keyed = med("a2. update_es, squitters") - med("a1. update, squitters"), med("a4. update_es with modes") - med("a3. update_modes")
        add_commb = med("a5. update_commb") - med("a3. update_modes")
        say(f"  update_es adds {1e3 * add_plain:.1f} us to update ({len(squitters)} frames, {1e6 * add_plain / len(squitters):.3f} ns per frame) "
            f"and {1e3 * add_keyed:.1f} us to update_modes ({n} frames, {1e6 * add_keyed / n:.3f} ns per frame); update_commb adds "
            f"{1e3 * add_commb:.1f} us to the same update_modes; the list has {int((out['flags'] & 2 != 0).sum())} position messages, "
            f"{int((out['flags'] & 4 != 0).sum())} of them resolved with a known version, {int((out['flags'] & 24 != 0).sum())} with a stale "
            f"supplement, {int((out['flags'] == 0).sum())} frames not counted")
        del de, desq, dc
    for t in tables:
        t.close()
    del df, dr, dsq
dem.close()
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as fh:
        fh.write("\n".join(lines) + "\n")
