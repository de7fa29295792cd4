#!/usr/bin/env python3
"""GPU box helper: device time of the Mode S stage (adsb_modes_of: modes_frames, the radix sort, the scan of the heads,
modes_heads, the scan of the squitters, modes_resolve, modes_totals) on a device-resident list of 2^20 frames of every
sort (tests/modes_cases.random_list) with 4096 known addresses in device memory, measured with device events on the ctx
stream, warm, one process:

  modes                   adsb_modes_of alone (no counts: nothing is copied from the host, nothing is waited for)
  wire input, for scale   adsb_wire_in_of(SHORT) over the same frames as one Beast stream in device memory
  host                    ONE CPU core: adsb_host_modes over the same list in host memory

  tools/gpu/modes_timing.py --out profiles/modes_timing.txt

The device's records, known_out, squitters and header are compared with the CPU mirror's, byte for byte."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1 << 20)
    ap.add_argument("--known", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", help="also write the report to this file")
    args = ap.parse_args()

    import numpy as np
    import torch

    import air_rs_amd as A
    from tests import modes_cases

    n = args.frames
    torch.cuda.set_stream(torch.cuda.Stream())  # a stream of our own: a NULL stream would make the ctx create one
    stream = torch.cuda.current_stream()
    dem = A.AdsbDemod(device=0, max_samples=1 << 16, max_out=1024, stream=stream.cuda_stream, host_staging=False)
    frames, pool = modes_cases.random_list(n, 2024, n_addresses=2 * args.known + 64)
    known = pool[:args.known].copy()
    assert len(known) == args.known
    dev_frames = torch.from_numpy(frames.view(np.uint8).reshape(-1).copy()).cuda()
    dev_known = torch.from_numpy(known.view(np.uint8).copy()).cuda()
    where, where_known = (dev_frames.data_ptr(), n), (dev_known.data_ptr(), len(known))
    beast, _ = dem.wire_of(frames)                       # every frame as a '3' frame: the same frames on the wire
    dev_beast = torch.from_numpy(np.frombuffer(beast, dtype=np.uint8).copy()).cuda()

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

    modes = timed(lambda: dem.modes_of_async(where, None, where_known))
    got = dem.fetch_modes()
    parse = timed(lambda: dem.wire_in_of_async((dev_beast.data_ptr(), len(beast)), filter="short"))
    parsed = int(dem.fetch_wire_in().header["n_frames"])
    assert parsed == n

    host_us = []
    for _ in range(3):
        t0 = time.perf_counter()
        mirror = A.host_modes(frames, None, known)
        host_us.append((time.perf_counter() - t0) * 1e6)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(got[:3], mirror[:3])) and got[4].tobytes() == mirror[4].tobytes(), \
        "device result != CPU mirror's"
    dem.close()
    hdr = got[4]
    host = float(np.median(host_us))
    text = (f"Mode S stage (adsb_modes_of), device time per call, median over {args.reps} repetitions after {args.warmup} warm ones\n"
            f"{n} frames and {len(known)} known addresses in device memory: " +
            ", ".join(f"{k[2:]} {int(hdr[k])}" for k in hdr.dtype.names[1:]) + "\n"
            f"{'modes':26s} {modes[0]:8.1f} us (min {modes[1]:.1f}, max {modes[2]:.1f}); {n / modes[0]:.1f} frames per us, "
            f"{56 * n / modes[0] / 1e3:.1f} GB/s of frames read and records written\n"
            f"{'wire input, for scale':26s} {parse[0]:8.1f} us (min {parse[1]:.1f}, max {parse[2]:.1f}): adsb_wire_in_of(SHORT) "
            f"over the same {n} frames as {len(beast)} bytes of Beast binary in device memory\n"
            f"{'one CPU core':26s} adsb_host_modes over the same list in host memory: median {host:.0f} us "
            f"(min {min(host_us):.0f}, 3 reps); device : host = 1 : {host / modes[0]:.0f}\n"
            "records, known_out, squitters and header of the device equal the CPU mirror's byte for byte\n")
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
