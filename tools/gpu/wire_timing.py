#!/usr/bin/env python3
"""GPU box helper: device time of the wire encoder (adsb_wire_device_async: three dispatches -- lengths, totals, encode
and write) on the frame list of the 1 GiB i8 bench buffer (synthetic input as bench.py makes it, HBM-resident), measured
with device events on the ctx stream, one process:

  beast + signal   the three kernels (the levels the signal byte needs are computed before the first event)
  avr              the same kernels with constant lengths
  levels           adsb_levels_device_async on the same list, for scale
  host             ONE CPU core: the device-to-host copy of the 24-byte frames and 32-byte level records, then
                   adsb_host_wire_encode over them (the alternative the device encoder stands against)

  tools/gpu/wire_timing.py --out profiles/wire_timing.txt

The stream of the first repetition is compared with the CPU mirror's, byte for byte.  Under a kernel trace
(rocprofv3 --kernel-trace --stats -- python tools/gpu/wire_timing.py --reps 20) the three kernels' own times appear as
wire_lengths, wire_totals and wire_write."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=1 << 29, help="i8 samples in the buffer (default: 1 GiB)")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", help="also write the report to this file")
    args = ap.parse_args()

    import numpy as np
    import torch

    import air_rs_amd as A

    n = args.samples
    torch.cuda.set_stream(torch.cuda.Stream())  # a stream of our own: a NULL stream would make the ctx create one
    stream = torch.cuda.current_stream()
    cfg = A.synth_default()
    cap = n // cfg.slot_len + 8192
    dem = A.AdsbDemod(device=0, sample_type=A.ADSB_SAMPLE_I8, max_samples=n, max_out=cap, stream=stream.cuda_stream,
                      host_staging=False)
    iq = torch.empty(n * 2, dtype=torch.int8, device="cuda")
    dem.synth_fill_device(cfg, 0, 0, n, iq.data_ptr())
    torch.cuda.synchronize()
    dem.timing_enable(1)
    dem.demod_device_async(iq.data_ptr(), n)
    n_frames = dem.fetch_counts()[0]

    def timed(call):
        """median, min, max in us of `call` alone between two events, the stream idle before the first"""
        ms = []
        for _ in range(args.warmup + args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record(stream)
            call()
            b.record(stream)
            b.synchronize()
            ms.append(a.elapsed_time(b))
        us = np.array(ms[args.warmup:]) * 1e3
        return float(np.median(us)), float(us.min()), float(us.max())

    levels = timed(dem.levels_async)                                  # (and the levels are current from here on)
    beast = timed(lambda: dem.wire_async("beast", signal=True))
    stream_bytes, ends = dem.fetch_wire()
    avr = timed(lambda: dem.wire_async("avr"))
    avr_bytes = len(dem.fetch_wire()[0])

    # one core: copy the records out, encode them
    t0 = time.perf_counter()
    frames = dem.fetch()[0]
    lv = dem.levels()
    t1 = time.perf_counter()
    host_us = []
    for _ in range(5):
        t2 = time.perf_counter()
        host_stream, host_ends = A.host_wire_encode(frames, lv)
        host_us.append((time.perf_counter() - t2) * 1e6)
    assert len(frames) == n_frames == len(ends)
    assert host_stream == stream_bytes and host_ends.tolist() == ends.tolist(), "device stream != CPU mirror's"
    scan_ms, finish_ms, _, n_timed = dem.timing_read3()
    dem.close()

    def line(name, t, nbytes):
        return (f"{name:24s} {t[0]:8.1f} us (min {t[1]:.1f}, max {t[2]:.1f}, {args.reps} reps)"
                + (f"; {nbytes / 1e6:.2f} MB of stream, {nbytes / t[0] / 1e3:.1f} GB/s written" if nbytes else "") + "\n")

    text = (f"wire encoder (adsb_wire_device_async), device time per call, median over the repetitions\n"
            f"i8, 1 x {n} samples, {n_frames} frames; scan {1e3 * scan_ms:.1f} us, finish_order {1e3 * finish_ms:.1f} us "
            f"({n_timed} launch)\n"
            + line("beast + signal, 3 kernels", beast, len(stream_bytes))
            + line("avr, 3 kernels", avr, avr_bytes)
            + line("levels kernel", levels, 0)
            + f"{'one CPU core':24s} copy of {n_frames} x (24 + 32) bytes to the host (adsb_fetch + adsb_fetch_levels, "
              f"with their waits and NumPy copies): {(t1 - t0) * 1e6:.0f} us; adsb_host_wire_encode (beast + signal): "
              f"median {np.median(host_us):.0f} us (min {min(host_us):.0f}, 5 reps)\n"
            + "the device stream equals the CPU mirror's byte for byte\n")
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
