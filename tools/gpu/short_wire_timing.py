#!/usr/bin/env python3
"""GPU box helper: device time of the level records by frame length (adsb_levels_modes_of) and of the wire output with
ADSB_WIRE_SHORT (adsb_wire_of), at 64 and 32 768 frames; device events on the ctx stream around each call, warm, median of
20, the calls of a group alternating.  Frame lists and level lists are in device memory; the level calls copy their
records to the host as adsb_levels_of does, except "device only" (out = NULL).

  levels   adsb_levels_modes_of on an all-long list beside two passes of adsb_levels_of on the same list (the same
           work: the two passes' distance from each other is the yardstick), then on an all-short list
  wire     adsb_wire_of with and without the bit, on an all-long list and on a mixed one

  tools/gpu/short_wire_timing.py --out out/short_wire_timing.txt     # (the recorded figures: profiles/short_wire_checks.txt)

Every timed result is compared with the CPU mirror's first, byte for byte."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--samples", type=int, default=1 << 24, help="samples of the buffer the frames lie in")
    ap.add_argument("--out", help="also write the report to this file")
    args = ap.parse_args()

    import numpy as np
    import torch

    import air_rs_amd as A

    torch.cuda.set_stream(torch.cuda.Stream())
    stream = torch.cuda.current_stream()
    n_samples = args.samples
    rng = np.random.default_rng(7)
    iq = rng.integers(-128, 128, size=(n_samples, 2)).astype(np.int8)
    dev = torch.from_numpy(iq.reshape(-1)).cuda()
    dem = A.AdsbDemod(device=0, max_samples=1 << 16, max_out=1 << 12, stream=stream.cuda_stream, host_staging=False)

    def frame_list(n, kind):
        fr = np.zeros(n, dtype=A.FRAME_DTYPE)
        fr["offset"] = np.sort(rng.integers(0, n_samples - 240, size=n)).astype(np.uint64)
        b = rng.integers(0, 256, size=(n, 14)).astype(np.uint8)
        short = {"long": np.zeros(n, bool), "short": np.ones(n, bool), "mixed": rng.integers(0, 2, size=n) == 0}[kind]
        b[:, 0] = np.where(short, 0x20, 0x8D)
        b[short, 7:] = 0
        fr["bytes"], fr["fixed_bit"] = b, 0xFF
        return fr

    def timed(calls):
        ms = [[] for _ in calls]
        for _ in range(args.warmup + args.reps):
            for k, call in enumerate(calls):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                a.record(stream)
                call()
                b.record(stream)
                b.synchronize()
                ms[k].append(a.elapsed_time(b))
        return [np.array(m[args.warmup:]) * 1e3 for m in ms]

    def line(name, us):
        return f"  {name:44s} {float(np.median(us)):9.1f} us (min {us.min():.1f}, max {us.max():.1f})\n"

    text = (f"level records by frame length and wire output with the short bit, i8, frames in {n_samples} samples of device "
            f"memory,\ndevice time per call (events on the ctx stream), median over {args.reps} alternating repetitions "
            f"after {args.warmup} warm ones\n")
    p = dev.data_ptr()
    for n in (64, 32768):
        text += f"{n} frames\n"
        long, short, mixed = frame_list(n, "long"), frame_list(n, "short"), frame_list(n, "mixed")
        dl, ds, dm = (torch.from_numpy(x.view(np.uint8).reshape(-1)).cuda() for x in (long, short, mixed))
        want_long = A.host_frame_levels_modes(iq, long)
        assert dem.levels_modes_of(p, n_samples, (dl.data_ptr(), n)).tobytes() == want_long.tobytes() == dem.levels_of(p, n_samples, (dl.data_ptr(), n)).tobytes()
        lv_short = dem.levels_modes_of(p, n_samples, (ds.data_ptr(), n))
        assert lv_short.tobytes() == A.host_frame_levels_modes(iq, short).tobytes()
        lv_mixed = dem.levels_modes_of(p, n_samples, (dm.data_ptr(), n))
        of1, modes, of2, shorts, dev_only = timed([
            lambda: dem.levels_of(p, n_samples, (dl.data_ptr(), n)),
            lambda: dem.levels_modes_of(p, n_samples, (dl.data_ptr(), n)),
            lambda: dem.levels_of(p, n_samples, (dl.data_ptr(), n)),
            lambda: dem.levels_modes_of(p, n_samples, (ds.data_ptr(), n)),
            lambda: dem.levels_modes_of(p, n_samples, (dl.data_ptr(), n), fetch=False)])
        text += (line("adsb_levels_of, all long, first pass", of1) + line("adsb_levels_of, all long, second pass", of2) +
                 line("adsb_levels_modes_of, all long", modes) + line("adsb_levels_modes_of, all long, device only", dev_only) +
                 line("adsb_levels_modes_of, all short", shorts))
        m1, m2, mm = float(np.median(of1)), float(np.median(of2)), float(np.median(modes))
        text += (f"  levels_modes_of / levels_of = {mm / min(m1, m2):.3f}; the two levels_of passes differ by "
                 f"{abs(m1 - m2) / min(m1, m2) * 100:.1f} %\n")
        dll, dlm = (torch.from_numpy(x.view(np.uint8).reshape(-1)).cuda() for x in (want_long, lv_mixed))
        for fmt in ("beast", "avr_mlat"):
            for short_bit in (False, True):
                assert dem.wire_of((dl.data_ptr(), n), dll.data_ptr(), format=fmt, short=short_bit)[0] == \
                    A.host_wire_encode(long, want_long, format=fmt, short=short_bit)[0]
                assert dem.wire_of((dm.data_ptr(), n), dlm.data_ptr(), format=fmt, short=short_bit)[0] == \
                    A.host_wire_encode(mixed, lv_mixed, format=fmt, short=short_bit)[0]
            got = timed([lambda: dem.wire_of((dl.data_ptr(), n), dll.data_ptr(), format=fmt),
                         lambda: dem.wire_of((dl.data_ptr(), n), dll.data_ptr(), format=fmt, short=True),
                         lambda: dem.wire_of((dm.data_ptr(), n), dlm.data_ptr(), format=fmt),
                         lambda: dem.wire_of((dm.data_ptr(), n), dlm.data_ptr(), format=fmt, short=True)])
            for name, us in zip(("all long, without the bit", "all long, with the bit", "mixed, without the bit",
                                 "mixed, with the bit"), got):
                text += line(f"adsb_wire_of {fmt}, {name}", us)
        del dl, ds, dm, dll, dlm
    dem.close()
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
