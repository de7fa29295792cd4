#!/usr/bin/env python3
"""GPU box helper: what the extended squitter status stage (adsb_es_of) costs beside the Comm-B stage (adsb_commb_of),
measured with device events on the ctx stream around each call alone, the same list in device memory for both, median of
20 after 5 warm-up calls, alternating in one process.

The two stages move the same 24 bytes in and 32 bytes out per frame through the same LDS staging and end with the same
one-workgroup fold, so the Comm-B stage is the like-for-like yardstick: what differs is the integer work per frame and
the number of counts per workgroup (14 against 12).  The list is a mix both stages find work in: the even frames from the
extended squitter tests' random list, the odd ones from the Comm-B tests'.  Each timed interval starts on an idle stream,
so it holds the launch latency of the two kernels it times.  `--frames N ...` (default 70 001 and 1 Mi); `--out PATH`
appends the report to PATH."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import air_rs_amd as A
from tests import commb_cases as KC
from tests import es_cases as KE

ap = argparse.ArgumentParser()
ap.add_argument("--out", help="append the report to this file")
ap.add_argument("--frames", type=int, nargs="*", default=[70_001, 1 << 20])
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


torch.cuda.set_stream(torch.cuda.Stream())  # a stream of our own: a NULL stream would make the ctx create one
stream = torch.cuda.current_stream().cuda_stream
say(f"==== extended squitter status stage beside the Comm-B stage: device {torch.cuda.get_device_name(0)}")
base = np.zeros(70_002, dtype=A.FRAME_DTYPE)
base[0::2], base[1::2] = KE.random_list(35_001, 99), KC.random_list(35_001, 99)
with A.AdsbDemod(device=0, stream=stream, host_staging=False, max_samples=1 << 16, max_out=1024) as d:
    for n in args.frames:
        frames = np.tile(base, (n + len(base) - 1) // len(base))[:n]
        dev = torch.from_numpy(frames.view(np.uint8).reshape(-1)).cuda()
        calls = {"adsb_es_of": lambda: d.es_of_async((dev.data_ptr(), n)),
                 "adsb_commb_of": lambda: d.commb_of_async((dev.data_ptr(), n))}
        got = {k: [] for k in calls}
        for rep in range(args.warmup + args.reps):                   # alternating: one of each per round
            for k, fn in calls.items():
                ms = timed_ms(fn)
                if rep >= args.warmup:
                    got[k].append(ms)
        check = min(n, len(base))
        (erecs, ehdr), (crecs, chdr) = d.fetch_es(), d.fetch_commb()
        assert erecs[:check].tobytes() == A.host_es(frames[:check])[0].tobytes() and int(ehdr["n"]) == n
        assert crecs[:check].tobytes() == A.host_commb(frames[:check])[0].tobytes() and int(chdr["n"]) == n
        say(f"{n} frames ({args.reps} alternating rounds after {args.warmup} warm-up rounds), "
            f"{n - int(ehdr['n_state'][0])} extended squitters, {int(chdr['n_commb'])} Comm-B replies:")
        for k, xs in got.items():
            say(f"  {k:<16s} {stats(xs)}")
        es, commb = (float(np.median(got[k])) for k in calls)
        say(f"  adsb_es_of / adsb_commb_of = {es / commb:.2f}; {56 * n / (es * 1e-3) / 1e9:.0f} GB/s of frames in and records out")
        del dev
if args.out:
    with open(args.out, "a") as fh:
        fh.write("\n".join(lines) + "\n")
