#!/usr/bin/env python3
"""GPU box helper: device time of the wire parser (adsb_wire_in_of: six dispatches -- last, carry, marks, totals, marks
again with the stores, counts) on the Beast stream of the frame list of the 1 GiB i8 bench buffer (synthetic input as
bench.py makes it; the stream is wire_of of the launch's frames with their levels and lies in device memory), measured
with device events on the ctx stream, one process:

  parse, beast + levels   the six kernels, the copy of the one stream end and the wait for it
  parse, beast + crc      the same with ADSB_WIRE_IN_CRC and no level records
  encoder                 adsb_wire_device_async on the same list, for scale
  host                    ONE CPU core: adsb_host_wire_parse over the same stream in host memory

  tools/gpu/wire_in_timing.py --out profiles/wire_in_timing.txt

The device's frames, rx, levels, counts, consumed and header are compared with the CPU mirror's, byte for byte."""
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
    dem.demod_device_async(iq.data_ptr(), n)
    frames = dem.fetch()[0]
    levels = dem.levels()
    beast, ends = dem.wire_of(frames, levels)
    dev = torch.from_numpy(np.frombuffer(beast, dtype=np.uint8).copy()).cuda()
    where = (dev.data_ptr(), len(beast))

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

    with_crc = timed(lambda: dem.wire_in_of_async(where, filter="crc"))
    n_crc = int(dem.fetch_wire_in().header["n_frames"])
    with_levels = timed(lambda: dem.wire_in_of_async(where, levels=True))
    got = dem.fetch_wire_in()
    encoder = timed(lambda: dem.wire_async("beast", signal=True))

    host_us = []
    for _ in range(5):
        t0 = time.perf_counter()
        mirror = A.host_wire_parse(beast, levels=True)
        host_us.append((time.perf_counter() - t0) * 1e6)
    same = all(x.tobytes() == y.tobytes() for x, y in zip(got, mirror))
    assert same, "device result != CPU mirror's"
    assert len(got.frames) == len(frames) and got.frames["bytes"].tobytes() == frames["bytes"].tobytes()
    assert got.rx["pos"].tolist() == [0] + ends[:-1].tolist()
    dem.close()

    def line(name, t):
        return (f"{name:26s} {t[0]:8.1f} us (min {t[1]:.1f}, max {t[2]:.1f}, {args.reps} reps); "
                f"{len(beast) / t[0] / 1e3:.2f} GB/s of stream, {len(frames) / t[0]:.1f} frames per us\n")

    text = (f"wire parser (adsb_wire_in_of), device time per call, median over the repetitions\n"
            f"i8, 1 x {n} samples, {len(frames)} frames as {len(beast)} bytes of Beast binary in device memory, one stream\n"
            + line("parse, beast + levels", with_levels)
            + line("parse, beast + crc filter", with_crc).rstrip("\n") + f"; {n_crc} frames pass\n"
            + f"{'encoder, for scale':26s} {encoder[0]:8.1f} us (min {encoder[1]:.1f}, max {encoder[2]:.1f}): "
              f"adsb_wire_device_async, beast + signal, on the launch's list\n"
            + f"{'one CPU core':26s} adsb_host_wire_parse (beast + levels) over the same bytes in host memory: median "
              f"{np.median(host_us):.0f} us (min {min(host_us):.0f}, 5 reps)\n"
            + "frames, rx, levels, counts, consumed and header of the device equal the CPU mirror's byte for byte\n")
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
