#!/usr/bin/env python3
"""GPU box helper: what clock sync costs (adsb_clock_sync_of, adsb_clock_apply), measured in one process with device
events on the ctx stream around the whole sync and around apply, warm, lists in device memory, medians with their range;
beside it the CPU mirror's time on one core.  Two lists of 32 768 position messages over 60 s: 6 receivers and 32
receivers, every message heard by all, 12 MHz ticks, offsets of 1 ms and drifts of 50 ppm.  `--out PATH` appends the
report to PATH (a run is meant to be kept as profiles/clock_timing.txt)."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import air_rs_amd as A
from tests import clock_cases as CC
from tests import mlat_cases as K
from tests import mlat_model as M
from tests.oracle_binding import Oracle

ap = argparse.ArgumentParser()
ap.add_argument("--out", help="append the report to this file")
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--messages", type=int, default=32768)
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


def big_list(oracle, n_rcv, n_msgs, seed):
    """n_msgs messages from 512 emitter positions in turn, heard by all n_rcv receivers; built with numpy, not message
    by message."""
    rng = np.random.default_rng(seed)
    rcv = K.receivers(n_rcv, seed=seed)
    pos, _ = K.emitters(oracle, 512, seed=seed + 1)
    frames = CC.position_frames(oracle, pos)
    st = np.array([M.ecef_of(r["latitude"], r["longitude"], r["height_m"]) for r in rcv])
    off, drift = rng.uniform(-1e-3, 1e-3, n_rcv), rng.uniform(-50e-6, 50e-6, n_rcv)
    t = np.sort(rng.uniform(0.5, 60.0, n_msgs))
    who = np.arange(n_msgs) % 512
    dist = np.sqrt(((pos[who][:, None, :] - st[None, :, :]) ** 2).sum(axis=2))
    ticks = np.floor((t[:, None] + dist / M.C_AIR + off[None, :] + drift[None, :] * t[:, None]) * 12e6).astype(np.int64) + 10 ** 9
    order = np.argsort(ticks, axis=1, kind="stable")
    recs = np.zeros(n_msgs * n_rcv, dtype=M.RECEPTION_DTYPE)
    recs["time"] = np.take_along_axis(ticks, order, axis=1).reshape(-1)
    recs["receiver"] = order.reshape(-1)
    recs["frame"] = np.arange(len(recs))
    rx = np.zeros(len(recs), dtype=M.WIRE_RX_DTYPE)
    rx["ticks"], rx["receiver"], rx["kind"] = recs["time"], recs["receiver"], ord("3")
    msgs = np.zeros(n_msgs, dtype=M.MESSAGE_DTYPE)
    msgs["bytes"] = np.array([np.frombuffer(f, dtype=np.uint8) for f in frames])[who]
    msgs["first"], msgs["n_receptions"] = np.arange(n_msgs) * n_rcv, n_rcv
    msgs["time"] = recs["time"][::n_rcv]
    return rcv, msgs, recs, rx


torch.cuda.set_stream(torch.cuda.Stream())  # a stream of our own: a NULL stream would make the ctx create one
stream = torch.cuda.current_stream().cuda_stream
say(f"==== clock sync timing: device {torch.cuda.get_device_name(0)}, {args.messages} messages, {args.reps} repetitions")
oracle = Oracle()
cfg = dict(time_source="ticks", seconds_per_time=1.0 / 12e6)
with A.AdsbDemod(device=0, stream=stream, host_staging=False, max_samples=1 << 16, max_out=1 << 12) as dem:
    for n_rcv in (6, 32):
        rcv, msgs, recs, rx = big_list(oracle, n_rcv, args.messages, seed=700 + n_rcv)
        dev = [torch.from_numpy(x.view(np.uint8).reshape(-1).copy()).cuda() for x in (msgs, recs, rx)]
        lists = [(d.data_ptr(), len(x)) for d, x in zip(dev, (msgs, recs, rx))]
        for label, extra in (("one pass", {}), ("two passes (max_residual_s = 1e-6)", dict(max_residual_s=1e-6))):
            kw = dict(cfg, **extra)
            run = lambda: dem.clock_sync_of_async(rcv, *lists, **kw)
            run()
            clocks, hdr = dem.fetch_clocks()
            sync = [timed_ms(run) for _ in range(args.reps)]
            dem.clock_apply_async()
            apply = [timed_ms(dem.clock_apply_async) for _ in range(args.reps)]
            t0 = time.perf_counter()
            mirror, _ = A.host_clock_sync(rcv, msgs, recs, rx, **kw)
            cpu = time.perf_counter() - t0
            same = all((clocks[k] == mirror[k]).all() for k in ("n_rows", "n_dropped", "n_partners", "flags"))
            say(f"  {n_rcv:2d} receivers, {label}: {int(hdr['n_rows'])} rows, {int(hdr['n_dropped'])} dropped, "
                f"{int(hdr['n_reached'])} reached; integer fields equal to the mirror's: {same}; largest offset gap "
                f"{np.abs(clocks['fine_offset_s'] - mirror['fine_offset_s']).max():.3g} s")
            say(f"     sync  {stats(sync)}  (includes the entry point's host work: stations, one copy, one wait)")
            say(f"     apply {stats(apply)}")
            say(f"     mirror on one CPU core: {1e3 * cpu:.1f} ms")
if args.out:
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")
