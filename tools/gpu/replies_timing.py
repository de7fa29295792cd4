#!/usr/bin/env python3
"""GPU box helper: device time of the replies scan (adsb_replies_of: replies_scan, replies_sums, replies_places,
replies_write) on the bench's synthetic buffer (1 GiB by default), i8 and CS16, beside the same process's product launch
on the same buffer (demod_tiles + finish_order) and that run's pure read of the buffer; device events on the ctx stream,
warm, median of 20, the two calls alternating:

  replies       adsb_replies_of alone, without the known filter (every address/parity candidate is written)
  product       adsb_demod_device_async alone (scan + finishing kernel)
  read          adsb_time_read_ceiling: the fastest of the read shapes over the same bytes

  tools/gpu/replies_timing.py --out out/replies_timing.txt     # (the recorded figures: profiles/replies_checks.txt, 6)

Reports the ratio of the replies scan to both.  On a smaller buffer (--check-samples) the device's list is compared with
the CPU mirror's, byte for byte."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=1 << 30, help="bytes of samples per buffer")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--check-samples", type=int, default=1 << 20, help="samples compared with the CPU mirror (0: none)")
    ap.add_argument("--out", help="also write the report to this file")
    args = ap.parse_args()

    import numpy as np
    import torch

    import air_rs_amd as A

    torch.cuda.set_stream(torch.cuda.Stream())  # a stream of our own: a NULL stream would make the ctx create one
    stream = torch.cuda.current_stream()
    text = (f"replies scan (adsb_replies_of) beside the product launch and the pure read, {args.bytes} bytes of synthetic samples "
            f"in device memory,\ndevice time per call, median over {args.reps} alternating repetitions after {args.warmup} warm ones\n")
    for name, st, bps in (("i8", A.ADSB_SAMPLE_I8, 2), ("CS16", A.ADSB_SAMPLE_I16, 4)):
        n = args.bytes // bps
        cfg = A.synth_default()
        if st == A.ADSB_SAMPLE_I16:
            cfg.amp_shift = 6
        cap = n // cfg.slot_len + 8192
        dem = A.AdsbDemod(device=0, sample_type=st, max_samples=n, max_out=cap, stream=stream.cuda_stream, host_staging=False)
        iq = torch.empty(n * bps, dtype=torch.int8, device="cuda")
        dem.synth_fill_device(cfg, 0, 0, n, iq.data_ptr())
        torch.cuda.synchronize()
        cap_replies = n // 4096                     # noise gives about one frame per 10 000 offsets

        def timed_pair(calls):
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

        replies, product = timed_pair([lambda: dem.replies_of_async(iq.data_ptr(), n_samples=n, max_frames=cap_replies),
                                       lambda: dem.demod_device_async(iq.data_ptr(), n)])
        frames, _, hdr = dem.fetch_replies()
        n_product = dem.fetch_counts()[0]
        read_us = dem.time_read_ceiling(iq.data_ptr(), n * bps, iters=10) * 1e3
        checked = "not compared"
        if args.check_samples:
            m = min(args.check_samples, n)
            got = dem.replies_of(iq.data_ptr(), n_samples=m, max_frames=cap_replies)
            host = np.frombuffer(iq[:m * bps].cpu().numpy().tobytes(), dtype=np.int8 if bps == 2 else np.int16).reshape(-1, 2)
            want = A.host_replies(host, max_frames=cap_replies)
            assert all(x.tobytes() == y.tobytes() for x, y in zip(got, want)), "device result != CPU mirror's"
            checked = f"list, counts and header of the first {m} samples equal the CPU mirror's byte for byte ({len(got[0])} frames)"
        dem.close()
        del iq
        r, p = float(np.median(replies)), float(np.median(product))
        text += (f"{name}: {n} samples; replies list {int(hdr['n_out'])} frames of {int(hdr['total_found'])} found "
                 f"({int(hdr['n_preamble'])} preambles, {int(hdr['n_all_call'])} DF11, {int(hdr['n_df18'])} DF18, "
                 f"{int(hdr['n_address_parity'])} address/parity, {int(hdr['n_parity'])} failed checks), flags {int(hdr['flags'])}; "
                 f"product list {n_product} frames\n"
                 f"  {'replies':10s} {r:9.1f} us (min {replies.min():.1f}, max {replies.max():.1f}); {args.bytes / r / 1e6:.2f} TB/s\n"
                 f"  {'product':10s} {p:9.1f} us (min {product.min():.1f}, max {product.max():.1f}); {args.bytes / p / 1e6:.2f} TB/s\n"
                 f"  {'read':10s} {read_us:9.1f} us; {args.bytes / read_us / 1e6:.2f} TB/s\n"
                 f"  replies / product = {r / p:.2f}; replies / read = {r / read_us:.2f}; product / read = {p / read_us:.2f}\n"
                 f"  {checked}\n")
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
