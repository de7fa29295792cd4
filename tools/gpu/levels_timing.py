#!/usr/bin/env python3
"""GPU box helper: device time of the per-frame levels kernel (adsb_levels_device_async: one wavefront per frame reads
the frame's 240 samples again), measured with device events on the ctx stream, beside the same run's scan and
finish_order times (adsb_timing_read3).  Synthetic input as bench.py makes it (default generator, HBM-resident):

  i8     1 GiB, one channel           cs16    1 GiB, one channel (amp_shift 6)
  i8x64  64 channels of 16 MiB        small   one 20 000-sample i8 buffer (the reference's buffer, adsb.rs:77-79)

  tools/gpu/levels_timing.py --config i8            # one configuration, one process
  tools/gpu/levels_timing.py --out profiles/levels_timing.txt
                                                    # all four, each in a child process of its own under `timeout`
Each repetition is one launch followed by one levels call; the levels call alone is between the two events (the launch
has finished before the first).  The records of the first repetition are compared with the CPU mirror on a slice."""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

CONFIGS = {  # name: (sample type, samples per channel, channels)
    "i8": ("i8", 1 << 29, 1),
    "cs16": ("i16", 1 << 28, 1),
    "i8x64": ("i8", 1 << 23, 64),
    "small": ("i8", 20_000, 1),
}
LIMIT_S = {"i8": 240, "cs16": 240, "i8x64": 240, "small": 120}


def run(name, reps, warmup):
    import numpy as np
    import torch

    import air_rs_amd as A

    kind, n, nch = CONFIGS[name]
    st, bps = (A.ADSB_SAMPLE_I8, 2) if kind == "i8" else (A.ADSB_SAMPLE_I16, 4)
    torch.cuda.set_stream(torch.cuda.Stream())  # a stream of our own: a NULL stream would make the ctx create one
    stream = torch.cuda.current_stream()
    cfg = A.synth_default()
    if st == A.ADSB_SAMPLE_I16:
        cfg.amp_shift = 6
    cap = n * nch // cfg.slot_len + 8192
    dem = A.AdsbDemod(device=0, sample_type=st, max_samples=n, max_out=cap, max_channels=nch,
                      stream=stream.cuda_stream, host_staging=False)
    iq = torch.empty(n * nch * bps, dtype=torch.int8, device="cuda")
    for c in range(nch):
        dem.synth_fill_device(cfg, c, 0, n, iq.data_ptr() + c * n * bps)
    torch.cuda.synchronize()

    def launch():
        dem.demod_device_async(iq.data_ptr(), n, n_channels=nch, channel_stride=n)

    ms = []
    dem.timing_enable(1)
    for rep in range(warmup + reps):
        launch()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record(stream)
        dem.levels_async()
        b.record(stream)
        b.synchronize()
        ms.append(a.elapsed_time(b))
        if rep == 0:   # the records are right: against the CPU mirror, channel 0's first frames
            frames, counts, total, flags = dem.fetch(max_out=256)
            lv = dem.levels(max_out=256)
            k = min(len(frames), counts[0])
            frames, lv = frames[:k], lv[:k]
            span = int(frames["offset"].max()) + A.WINDOW if k else 0
            host = iq[:span * bps].cpu().numpy().view(np.int8 if bps == 2 else np.int16).reshape(-1, 2)
            assert flags & ~A.ADSB_FLAG_TRUNCATED == 0 and lv.tobytes() == A.host_frame_levels(host, frames).tobytes(), name
    scan_ms, finish_ms, _, n_timed = dem.timing_read3()
    n_frames = dem.fetch_counts()[0]
    ms = np.array(ms[warmup:]) * 1e3
    moved = n_frames * (240 * bps + 56)
    print(f"{name:6s} {kind} {nch:3d} x {n:10d} samples, {n_frames:7d} frames: levels {np.median(ms):8.1f} us "
          f"(min {ms.min():.1f}, max {ms.max():.1f}, {len(ms)} reps; {moved / 1e6:.1f} MB, "
          f"{moved / np.median(ms) / 1e3:.0f} GB/s) | scan {1e3 * scan_ms:8.1f} us, finish_order {1e3 * finish_ms:6.1f} us "
          f"({n_timed} launches)", flush=True)
    dem.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=sorted(CONFIGS), help="run this configuration in this process")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", help="also write the report to this file")
    args = ap.parse_args()
    if args.config:
        run(args.config, max(args.reps, 20), max(args.warmup, 1))
        return 0
    lines = ["levels kernel (adsb_levels_device_async), device time per call, median over the repetitions\n"]
    print(lines[0], end="", flush=True)
    for name in ("i8", "cs16", "i8x64", "small"):   # every configuration a fresh process with a time limit of its own
        cmd = ["timeout", "-k", "10", str(LIMIT_S[name]), sys.executable, os.path.abspath(__file__), "--config", name,
               "--reps", str(args.reps), "--warmup", str(args.warmup)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        lines.append(r.stdout)
        if r.returncode != 0:                       # nothing more on this GPU after a failure
            sys.stderr.write(r.stderr[-4000:])
            print(f"{name}: exit status {r.returncode}; stopping", flush=True)
            return r.returncode
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
