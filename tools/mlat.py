#!/usr/bin/env python3
"""Where were these messages sent from?  Beast recordings of R receivers -> wire input -> correlate -> multilaterate,
all on the device (or, with --host, through the CPU mirrors of the three steps).

  tools/mlat.py SITES.csv A.beast B.beast ...

SITES.csv has one line per recording, in the same order: latitude,longitude,height_m[,clock_offset_s] (degrees, metres
above the ellipsoid, seconds the receiver's 12 MHz clock is ahead of true time); '#' starts a comment.  One line per
valid fix: time of the first reception in seconds of its receiver's clock, ICAO address, latitude, longitude, height in
metres, residual in metres, hdop, receivers used.

--sync first estimates every receiver's clock offset and drift against receiver --reference from the position messages
of the recordings themselves (clock sync; the clock_offset_s column is then the prior, good enough for correlate's
window), prints one '# clock' line per receiver, and solves the fixes from the corrected times."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def read_sites(path):
    sites = []
    for line in open(path):
        line = line.split("#")[0].strip()
        if line:
            v = [float(x) for x in line.split(",")]
            if len(v) not in (3, 4):
                raise SystemExit(f"{path}: want latitude,longitude,height_m[,clock_offset_s], got {line!r}")
            sites.append(tuple(v))
    return sites


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("sites")
    ap.add_argument("recordings", nargs="+")
    ap.add_argument("--window", type=int, default=2400, help="correlate window in 2 MHz samples (default 1.2 ms)")
    ap.add_argument("--no-altitude", action="store_true", help="do not use the messages' own altitudes")
    ap.add_argument("--max-residual", type=float, default=0.0, help="reject fixes with a larger residual, metres")
    ap.add_argument("--host", action="store_true", help="CPU mirrors instead of the device")
    ap.add_argument("--sync", action="store_true", help="estimate the receivers' clocks first and solve from corrected times")
    ap.add_argument("--reference", type=int, default=0, help="with --sync: the receiver whose clock is taken as true")
    ap.add_argument("--max-residual-us", type=float, default=0.0,
                    help="with --sync: a second pass without the rows whose residual is larger, microseconds")
    args = ap.parse_args()

    import numpy as np

    import air_rs_amd as A

    sites = read_sites(args.sites)
    if len(sites) != len(args.recordings):
        raise SystemExit(f"{len(sites)} sites for {len(args.recordings)} recordings")
    streams = [open(p, "rb").read() for p in args.recordings]
    data, ends = b"".join(streams), np.cumsum([len(s) for s in streams])
    cfg = dict(time_source="ticks", use_altitude=not args.no_altitude, max_residual_m=args.max_residual)
    # wire input's frame offsets are 2 MHz samples: the unit of the messages' own times
    sync = dict(reference=args.reference, max_residual_s=args.max_residual_us * 1e-6, seconds_per_time=0.5e-6)
    clocks = None
    if args.host:
        win = A.host_wire_parse(data, ends, filter=["crc", "df17"])
        msgs, _, recs = A.host_correlate(win.frames, win.counts, args.window)
        if args.sync:
            clocks, _ = A.host_clock_sync(sites, msgs, recs, win.rx, time_source="ticks", **sync)
            corrected = A.host_clock_apply(clocks, msgs, recs, win.rx, time_source="ticks", **sync)
            plain = [s[:3] for s in sites]
            fixes, hdr = A.host_multilaterate(plain, msgs, corrected, **dict(cfg, time_source="reception",
                                                                              seconds_per_tick=1 / 12e6 / 256))
        else:
            fixes, hdr = A.host_multilaterate(sites, msgs, recs, win.rx, **cfg)
    elif args.sync:
        with A.AdsbDemod(max_samples=1 << 16, max_out=1024) as d:
            win = d.wire_in_of(data, ends, filter=["crc", "df17"])
            d.correlate_of_async((d.wire_in_device()[0], len(win.frames)), win.counts, args.window)
            fixes, hdr = d.multilaterate(sites, rx=d.wire_in_device()[1], clocks=True, clock_cfg=sync, **cfg)
            clocks, _ = d.fetch_clocks()
            msgs, _, recs = d.fetch_correlated()
    else:
        with A.AdsbDemod(max_samples=1 << 16, max_out=1024) as d:
            win = d.wire_in_of(data, ends, filter=["crc", "df17"])
            d.correlate_of_async((d.wire_in_device()[0], len(win.frames)), win.counts, args.window)
            fixes, hdr = d.multilaterate(sites, rx=d.wire_in_device()[1], **cfg)   # behind correlate, nothing fetched
            msgs, _, recs = d.fetch_correlated()
    for r, k in enumerate(clocks if clocks is not None else ()):
        what = "reference" if k["flags"] & A.ADSB_CLOCK_REFERENCE else "reached" if k["flags"] & A.ADSB_CLOCK_REACHED \
            else "unreached"
        print(f"# clock {r:3d} {what:9s} offset {k['offset_s']:+.9f} s drift {k['drift'] * 1e6:+9.3f} ppm "
              f"rms {k['residual_rms_s'] * 1e9:8.1f} ns rows {int(k['n_rows'])} dropped {int(k['n_dropped'])}")
    for m, f in zip(msgs, fixes):
        if f["flags"] & A.ADSB_MLAT_VALID:
            t = int(win.rx["ticks"][recs["frame"][m["first"]]]) / 12e6
            icao = int(m["bytes"][1]) << 16 | int(m["bytes"][2]) << 8 | int(m["bytes"][3])
            print(f"{t:14.6f} {icao:06X} {f['latitude']:10.5f} {f['longitude']:11.5f} {f['height_m']:8.0f} "
                  f"{f['residual_rms_m']:8.1f} {f['hdop']:6.1f} {int(f['n_used']):3d}")
    print(f"# {int(hdr['n_messages'])} messages, {int(hdr['n_attempted'])} attempted, {int(hdr['n_valid'])} valid",
          file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
