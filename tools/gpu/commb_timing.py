#!/usr/bin/env python3
"""GPU box helper: what the Comm-B stage (adsb_commb_of) costs, measured with device events on the ctx stream around the
call alone, list in device memory, median of 20 after 5 warm-up calls, beside a device-to-device copy in the same run.

The stage is one read of 24 bytes and one write of 32 bytes per frame.  The yardstick the checks file asks for is a
device-to-device copy of the same 24 + 32 = 56 bytes per frame; such a copy reads AND writes every byte, so it moves 112
bytes per frame over the memory bus where the stage moves 56, and a copy of 28 bytes per frame (the same traffic as the
stage) is timed too.  Each timed interval starts on an idle stream, so it holds the launch latency of what it times:
two kernels for the stage, one for a copy.  `--frames N` (default 1 Mi, then 8 Mi to tell the fixed cost from the cost
per frame); `--out PATH` appends the report to PATH."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import air_rs_amd as A
from tests import commb_cases as K

ap = argparse.ArgumentParser()
ap.add_argument("--out", help="append the report to this file")
ap.add_argument("--frames", type=int, nargs="*", default=[1 << 20, 1 << 23])
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
say(f"==== Comm-B stage: device {torch.cuda.get_device_name(0)}")
base = K.random_list(1 << 16, 17)                                    # the tests' mix, repeated
with A.AdsbDemod(device=0, stream=stream, host_staging=False, max_samples=1 << 16, max_out=1024) as d:
    for n in args.frames:
        frames = np.tile(base, (n + len(base) - 1) // len(base))[:n]
        dev = torch.from_numpy(frames.view(np.uint8).reshape(-1)).cuda()
        src, dst = torch.empty(56 * n, dtype=torch.uint8, device="cuda"), torch.empty(56 * n, dtype=torch.uint8, device="cuda")
        src.fill_(1)
        calls = {"adsb_commb_of": lambda: d.commb_of_async((dev.data_ptr(), n)),
                 "copy of 56 bytes per frame": lambda: dst.copy_(src),
                 "copy of 28 bytes per frame": lambda: dst[:28 * n].copy_(src[:28 * n])}
        got = {k: [] for k in calls}
        for rep in range(args.warmup + args.reps):                   # alternating: one of each per round
            for k, fn in calls.items():
                ms = timed_ms(fn)
                if rep >= args.warmup:
                    got[k].append(ms)
        recs, hdr = d.fetch_commb()
        want = A.host_commb(frames[:1 << 16])
        assert recs[:1 << 16].tobytes() == want[0].tobytes() and int(hdr["n"]) == n
        say(f"{n} frames ({args.reps} alternating rounds after {args.warmup} warm-up rounds), n_one {int(hdr['n_one'])}, "
            f"n_ambiguous {int(hdr['n_ambiguous'])}:")
        for k, xs in got.items():
            say(f"  {k:<28s} {stats(xs)}")
        stage, c56, c28 = (float(np.median(got[k])) for k in calls)
        say(f"  stage / copy of 56 B per frame = {stage / c56:.2f}; stage / copy of 28 B per frame (equal traffic) = {stage / c28:.2f}; "
            f"{56 * n / (stage * 1e-3) / 1e9:.0f} GB/s of frames in and records out")
        del dev, src, dst
if args.out:
    with open(args.out, "a") as fh:
        fh.write("\n".join(lines) + "\n")
