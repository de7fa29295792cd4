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
window), prints one '# clock' line per receiver, and solves the fixes from the corrected times.

--aircraft feeds the correlated messages and their fixes into a track table (on the device where they lie; with --host
through the CPU mirror of the per-frame step and a plain merge) and prints, instead of the fixes, one line per aircraft:
ICAO, callsign, the position it reports, the multilaterated position, the age of that fix at the last message, pdop,
valid/attempted fixes, checked/disagreeing position messages, and the largest disagreement in metres.
--max-disagreement M (default 1000): how far a reported position may lie from the solved one.

--modes also places aircraft that send no ADS-B: the recordings are parsed with their 56-bit frames and without the CRC
and DF17 filters (ADSB_WIRE_IN_SHORT), every correlated message gets its address from the Mode S stage (adsb_modes_of
on correlate's frames_out: DF11 all-call replies teach an address, DF0/4/5/16/20/21 replies carry theirs on the parity),
and only messages whose address is an aircraft's (kinds SELF and KNOWN) are printed, with that address.  On the device
every step reads the one before where it lies: correlate's frames go to the Mode S stage, every message to the solver,
and nothing is fetched before the end; --host solves the messages with an address only.  Not with --sync.

--modes --aircraft: the table takes frames, Mode S records and fixes in one update (adsb_track_table_update_modes), so
an aircraft that only answers interrogations has a row, keyed by the address the Mode S stage gave its replies, with its
multilaterated position.  Five columns are appended: Alt(S), Squawk and Call(S) from its newest replies that carry them,
Replies (DF0/4/5/11/16/20/21 frames counted), and S, which is "S" for an aircraft that has sent no DF17/18 frame.

--modes --commb --aircraft: the Comm-B stage (adsb_commb_of) reads the same frames where they lie and the table takes its
records too (adsb_track_table_update_commb): per aircraft the newest BDS 4,0, 5,0 and 6,0, a reply that reads as 5,0 and
as 6,0 settled from the aircraft's own ADS-B velocity.  Six more columns: SelAlt, QNH, GS/Trk(B), Hdg, IAS, Mach, with a
"*" behind a value from a settled reply.

--modes --es --aircraft: the extended squitter status stage (adsb_es_of) reads the same frames and the table takes its
records too (adsb_track_table_update_es, on the keyed path): NIC and Rc of each aircraft's newest position message resolved
with the version and NIC supplements of its own operational status messages.  Eight more columns: Ver, NIC, Rc, NACp, SIL,
Emerg, Squawk(ES), SelAlt, with a "?" behind NIC and Rc where no version was known when the position was heard.

--aircraft --filter: the table also runs every aircraft's fixes through its Kalman filter (adsb_track_table_filter_reserve;
with --host the CPU mirror of its two steps), so an aircraft that sends no ADS-B has a speed and a track too.  Six columns
are appended last: Lat(f), Lon(f) (the filtered position), GS(f) in knots, Trk(f) in degrees, VR(f) in ft/min (n/a until
the filter has seen min_run fixes in a row) and Outl, the fixes it turned away."""
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


def host_table(A, frames, fixes, max_disagreement, modes=None, filt=False):
    """What a table with an mlat reserve makes of the list, without a device: the CPU tracker for the records, the CPU
    mirror of the per-frame step and the header's merge rules (saturating add, max, newest by position) for the mlat
    records -> (AIRCRAFT_DTYPE records, AIRCRAFT_MLAT_DTYPE records), ascending ICAO.  modes (the frames' MODES_DTYPE
    records): what update_modes makes of it instead -- frames that are not SELF or KNOWN are skipped, the others are
    keyed by their address, a frame that is no DF17/18 is one of kind "other" to the tracker -- and a third array, the
    AIRCRAFT_MODES_DTYPE records by the CPU mirror of the modes step and its combine.  filt: a last array, the
    AIRCRAFT_FILTER_DTYPE records by the CPU mirror of the filter's operand and step."""
    import numpy as np
    tracker, state, count, side, track = A.Tracker(), {}, {}, {}, {}
    sat = (1 << 32) - 1
    for j, (fr, fx) in enumerate(zip(frames, fixes)):
        b = fr["bytes"].tobytes()
        time = float(int(fr["offset"])) * 0.5e-6
        icao = b[1] << 16 | b[2] << 8 | b[3]
        seen = b
        if modes is not None:
            if int(modes[j]["kind"]) > A.ADSB_MODES_KNOWN:
                continue
            icao = int(modes[j]["address"]) & 0xFFFFFF
            if int(modes[j]["df"]) not in (17, 18):                      # no ADS-B message, whatever byte 4 looks like
                seen = bytes([17 << 3, icao >> 16, icao >> 8 & 0xFF, icao & 0xFF]) + bytes(10)
            one_side = A.host_track_modes_of(modes[j], time)[0]
            side[icao] = A.host_track_modes_merge(side[icao], one_side) if icao in side else one_side
        tracker.update(seen, time)
        count[icao] = count.get(icao, 0) + 1
        one = A.host_track_mlat_of(max_disagreement, b, fx, time)[0]
        if filt:
            track[icao] = A.host_track_filter_step(track[icao] if icao in track else A.filter_empty()[0],
                                                   A.host_track_filter_operand(fx, time))[0]
        a = state.get(icao)
        if a is None:
            a = np.zeros((), dtype=A.AIRCRAFT_MLAT_DTYPE)
            a["time"] = np.nan
        for name in ("n_attempted", "n_valid", "n_checked", "n_disagree"):
            a[name] = min(int(a[name]) + int(one[name]), sat)
        if one["flags"] & A.ADSB_TRACK_MLAT_VALID:
            for name in ("time", "latitude", "longitude", "height_m", "residual_rms_m", "pdop", "n_used"):
                a[name] = one[name]
            a["flags"] = (int(a["flags"]) & A.ADSB_TRACK_MLAT_CHECKED) | \
                (int(one["flags"]) & (A.ADSB_TRACK_MLAT_VALID | A.ADSB_TRACK_MLAT_ALTITUDE))
        if one["flags"] & A.ADSB_TRACK_MLAT_CHECKED:
            a["last_disagreement_m"] = one["last_disagreement_m"]
            a["max_disagreement_m"] = max(a["max_disagreement_m"], one["max_disagreement_m"])
            a["flags"] = int(a["flags"]) | A.ADSB_TRACK_MLAT_CHECKED
        state[icao] = a
    recs = np.zeros(len(state), dtype=A.AIRCRAFT_DTYPE)
    mlat = np.zeros(len(state), dtype=A.AIRCRAFT_MLAT_DTYPE)
    for k, icao in enumerate(sorted(state)):
        s = tracker.get(icao)
        recs[k] = (s.latitude, s.longitude, s.last_contact, icao, s.altitude, 1 if s.has_position else 0, count[icao],
                   s.callsign)
        mlat[k] = state[icao]
    out = (recs, mlat)
    if modes is not None:
        out += (np.array([side[icao] for icao in sorted(state)], dtype=A.AIRCRAFT_MODES_DTYPE),)
    if filt:
        out += (np.array([track[icao] for icao in sorted(state)], dtype=A.AIRCRAFT_FILTER_DTYPE),)
    return out


def modes_columns(A, s):
    """Alt(S), Squawk, Call(S), Replies and S of one AIRCRAFT_MODES_DTYPE record."""
    flags = int(s["flags"])
    return "\t".join([f"{int(s['altitude_ft'])}" if flags & A.ADSB_TRACK_MODES_ALT else "n/a",
                      f"{int(s['squawk']):04d}" if flags & A.ADSB_TRACK_MODES_SQUAWK else "n/a",
                      (s["callsign"].decode("ascii", "replace").replace("_", " ").strip() or "n/a")
                      if flags & A.ADSB_TRACK_MODES_CALLSIGN else "n/a",
                      f"{int(s['n_replies'])}", "" if flags & A.ADSB_TRACK_MODES_SQUITTER else "S"])


def filter_columns(A, f):
    """Lat(f), Lon(f), GS(f), Trk(f), VR(f) and Outl of one AIRCRAFT_FILTER_DTYPE record."""
    flags = int(f["flags"])
    p = A.filter_physical(f)[0]
    place = f"{float(f['latitude']):.5f}\t{float(f['longitude']):.5f}" if flags & A.ADSB_TRACK_FILTER_RUNNING else "n/a\tn/a"
    moving = (f"{p['ground_speed_kt']:.0f}\t{p['track_deg']:.0f}\t{p['vertical_rate_fpm']:.0f}"
              if flags & A.ADSB_TRACK_FILTER_VELOCITY else "n/a\tn/a\tn/a")
    return f"{place}\t{moving}\t{int(f['n_outlier'])}"


def aircraft_lines(A, recs, mlat, now, modes=None, commb=None, es=None, filt=None):
    """One tab-separated line per aircraft, under a header line.  modes (AIRCRAFT_MODES_DTYPE records): five more
    columns.  commb (AIRCRAFT_COMMB_DTYPE records): six more.  es (aircraft_es_columns' rows): eight more.  filt
    (AIRCRAFT_FILTER_DTYPE records): six more, last."""
    out = ("ICAO\tCallsign\tLatitude\tLongitude\tMlatLat\tMlatLon\tAge\tPdop\tValid/Attempted\tChecked/Disagree"
           "\tMaxDisagreement" + ("" if modes is None else "\tAlt(S)\tSquawk\tCall(S)\tReplies\tS")
           + ("" if commb is None else "\t" + "\t".join(A.AIRCRAFT_COMMB_COLUMNS))
           + ("" if es is None else "\t" + "\t".join(A.AIRCRAFT_ES_COLUMNS))
           + ("" if filt is None else "\tLat(f)\tLon(f)\tGS(f)\tTrk(f)\tVR(f)\tOutl") + "\n")
    registers = None if commb is None else A.aircraft_commb_columns(commb)
    for k, (r, m) in enumerate(zip(recs, mlat)):
        call = r["callsign"].decode("ascii", "replace").strip() or "n/a"
        said = f"{float(r['latitude']):.5f}\t{float(r['longitude']):.5f}" if r["has_position"] else "n/a\tn/a"
        if m["flags"] & A.ADSB_TRACK_MLAT_VALID:
            solved = (f"{float(m['latitude']):.5f}\t{float(m['longitude']):.5f}\t{now - float(m['time']):.1f}"
                      f"\t{float(m['pdop']):.1f}")
        else:
            solved = "n/a\tn/a\tn/a\tn/a"
        worst = f"{float(m['max_disagreement_m']):.0f}" if m["flags"] & A.ADSB_TRACK_MLAT_CHECKED else "n/a"
        out += (f"{int(r['icao']):06X}\t{call}\t{said}\t{solved}\t{int(m['n_valid'])}/{int(m['n_attempted'])}"
                f"\t{int(m['n_checked'])}/{int(m['n_disagree'])}\t{worst}"
                + ("" if modes is None else "\t" + modes_columns(A, modes[k]))
                + ("" if registers is None else "\t" + "\t".join(registers[k]))
                + ("" if es is None else "\t" + "\t".join(es[k]))
                + ("" if filt is None else "\t" + filter_columns(A, filt[k])) + "\n")
    return out


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
    ap.add_argument("--aircraft", action="store_true", help="one line per aircraft instead of one per fix")
    ap.add_argument("--max-disagreement", type=float, default=1000.0,
                    help="with --aircraft: metres a reported position may lie from the multilaterated one")
    ap.add_argument("--modes", action="store_true", help="Mode S replies too: short frames, addresses from the Mode S stage")
    ap.add_argument("--commb", action="store_true",
                    help="with --modes --aircraft: the aircraft's Comm-B registers too, six more columns")
    ap.add_argument("--es", action="store_true",
                    help="with --modes --aircraft: the aircraft's extended squitter status too, NIC and Rc resolved per "
                         "aircraft, eight more columns")
    ap.add_argument("--filter", action="store_true",
                    help="with --aircraft: each aircraft's fixes through the table's Kalman filter, six more columns")
    ap.add_argument("--max-iterations", type=int, default=0,
                    help="the solver's step limit (default: its own, 24); replies carry no altitude, and a free solve over "
                         "ground receivers may need 200")
    args = ap.parse_args()
    if args.modes and args.sync:
        ap.error("--modes does not go with --sync")
    if args.commb and not (args.modes and args.aircraft):
        ap.error("--commb needs --modes and --aircraft")
    if args.es and not (args.modes and args.aircraft):
        ap.error("--es needs --modes and --aircraft")
    if args.filter and not args.aircraft:
        ap.error("--filter needs --aircraft")

    import numpy as np

    import air_rs_amd as A

    sites = read_sites(args.sites)
    if len(sites) != len(args.recordings):
        raise SystemExit(f"{len(sites)} sites for {len(args.recordings)} recordings")
    streams = [open(p, "rb").read() for p in args.recordings]
    data, ends = b"".join(streams), np.cumsum([len(s) for s in streams])
    cfg = dict(time_source="ticks", use_altitude=not args.no_altitude, max_residual_m=args.max_residual,
               max_iterations=args.max_iterations)
    # wire input's frame offsets are 2 MHz samples: the unit of the messages' own times
    sync = dict(reference=args.reference, max_residual_s=args.max_residual_us * 1e-6, seconds_per_time=0.5e-6)
    clocks = None
    aircraft = None

    def table_of(d, n_msgs):
        """The correlated messages and their fixes, where they lie on the device, into a table -> (records, mlat)"""
        with A.TrackTable(d, max_frames=max(n_msgs, 1), seconds_per_sample=0.5e-6) as table:
            table.mlat_reserve(args.max_disagreement)
            if args.filter:
                table.filter_reserve()
            table.update_device(d.correlated_device()[1], n_msgs, 0, mlat_ptr=d.mlat_device()[0])
            return (table.aircraft()[0], table.mlat()) + ((table.filter(),) if args.filter else ())

    def resolved(msgs, recs, modes):
        """The messages whose address is an aircraft's, with their receptions -> (messages, receptions, addresses)"""
        keep = np.flatnonzero(modes["kind"] <= A.ADSB_MODES_KNOWN)
        out = msgs[keep].copy()
        parts = [recs[int(m["first"]):int(m["first"]) + int(m["n_receptions"])] for m in out]
        out["first"] = np.cumsum([0] + [len(p) for p in parts])[:-1]
        return out, (np.concatenate(parts) if parts else recs[:0]), modes["address"][keep]

    address = accepted = newest = commb_side = es_side = None
    if args.modes and args.host:
        win = A.host_wire_parse(data, ends, filter="short")
        every, fout, recs = A.host_correlate(win.frames, win.counts, args.window)
        mrec = A.host_modes(fout)[0]
        msgs, recs, address = resolved(every, recs, mrec)
        fixes, hdr = A.host_multilaterate(sites, msgs, recs, win.rx, **cfg)
        if args.aircraft:
            spread = np.zeros(len(every), dtype=A.MLAT_FIX_DTYPE)       # a fix per message: none where none was solved
            spread[np.flatnonzero(mrec["kind"] <= A.ADSB_MODES_KNOWN)] = fixes
            aircraft = host_table(A, fout, spread, args.max_disagreement, modes=mrec, filt=args.filter)
            if args.commb:                                              # every accepted address has a row in both
                commb_side = A.host_track_commb(fout, mrec, A.host_commb(fout)[0])[1]
            if args.es:
                es_side = A.aircraft_es_columns(A.host_track_es(fout, A.host_es(fout)[0], mrec)[1])
            newest = float(int(every["time"][-1])) * 0.5e-6 if len(every) else 0.0
    elif args.modes:
        with A.AdsbDemod(max_samples=1 << 16, max_out=1024) as d:
            win = d.wire_in_of(data, ends, filter="short")
            d.correlate_of_async((d.wire_in_device()[0], len(win.frames)), win.counts, args.window)
            n_msgs = d.correlated_counts()[0]                            # the solver and the Mode S stage take it from the host
            d.modes_of_async((d.correlated_device()[1], n_msgs))         # behind correlate, on its frames where they lie
            d.multilaterate_async(sites, rx=d.wire_in_device()[1], **cfg)   # every message; the table takes the accepted ones
            if args.aircraft:
                with A.TrackTable(d, max_frames=max(n_msgs, 1), seconds_per_sample=0.5e-6) as table:
                    table.mlat_reserve(args.max_disagreement)
                    table.modes_reserve()
                    if args.filter:
                        table.filter_reserve()
                    commb_ptr = None
                    if args.commb:
                        table.commb_reserve()
                        d.commb_of_async((d.correlated_device()[1], n_msgs))     # the same frames, where they lie
                        commb_ptr = d.commb_device()[0]
                    es_ptr = None
                    if args.es:
                        table.es_reserve()
                        d.es_of_async((d.correlated_device()[1], n_msgs))        # likewise
                        es_ptr = d.es_device()[0]
                    table.update_device(d.correlated_device()[1], n_msgs, 0, mlat_ptr=d.mlat_device()[0],
                                        modes_ptr=d.modes_device()[0], commb_ptr=commb_ptr, es_ptr=es_ptr)
                    aircraft = (table.aircraft()[0], table.mlat(), table.modes()) + ((table.filter(),) if args.filter else ())
                    commb_side = table.commb() if args.commb else None
                    es_side = A.aircraft_es_columns(table.es()) if args.es else None
            fixes, hdr = d.fetch_mlat()
            msgs, _, recs = d.fetch_correlated()
            mrec = d.fetch_modes()[0]
            address, accepted = mrec["address"], mrec["kind"] <= A.ADSB_MODES_KNOWN
    elif args.host:
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
        if args.aircraft:
            aircraft = host_table(A, A.frames_of_messages(msgs), fixes, args.max_disagreement, filt=args.filter)
    elif args.sync:
        with A.AdsbDemod(max_samples=1 << 16, max_out=1024) as d:
            win = d.wire_in_of(data, ends, filter=["crc", "df17"])
            d.correlate_of_async((d.wire_in_device()[0], len(win.frames)), win.counts, args.window)
            fixes, hdr = d.multilaterate(sites, rx=d.wire_in_device()[1], clocks=True, clock_cfg=sync, **cfg)
            clocks, _ = d.fetch_clocks()
            msgs, _, recs = d.fetch_correlated()
            if args.aircraft:
                aircraft = table_of(d, len(msgs))
    else:
        with A.AdsbDemod(max_samples=1 << 16, max_out=1024) as d:
            win = d.wire_in_of(data, ends, filter=["crc", "df17"])
            d.correlate_of_async((d.wire_in_device()[0], len(win.frames)), win.counts, args.window)
            fixes, hdr = d.multilaterate(sites, rx=d.wire_in_device()[1], **cfg)   # behind correlate, nothing fetched
            msgs, _, recs = d.fetch_correlated()
            if args.aircraft:
                aircraft = table_of(d, len(msgs))
    for r, k in enumerate(clocks if clocks is not None else ()):
        what = "reference" if k["flags"] & A.ADSB_CLOCK_REFERENCE else "reached" if k["flags"] & A.ADSB_CLOCK_REACHED \
            else "unreached"
        print(f"# clock {r:3d} {what:9s} offset {k['offset_s']:+.9f} s drift {k['drift'] * 1e6:+9.3f} ppm "
              f"rms {k['residual_rms_s'] * 1e9:8.1f} ns rows {int(k['n_rows'])} dropped {int(k['n_dropped'])}")
    if aircraft is not None:
        if newest is None:
            newest = float(int(msgs["time"][-1])) * 0.5e-6 if len(msgs) else 0.0
        filter_side = aircraft[-1] if args.filter else None
        print(aircraft_lines(A, aircraft[0], aircraft[1], newest, aircraft[2] if args.modes else None, commb_side,
                             es_side, filter_side), end="")
    for k, (m, f) in enumerate(zip(msgs, fixes)):
        if aircraft is None and f["flags"] & A.ADSB_MLAT_VALID and (accepted is None or accepted[k]):
            t = int(win.rx["ticks"][recs["frame"][m["first"]]]) / 12e6
            icao = int(m["bytes"][1]) << 16 | int(m["bytes"][2]) << 8 | int(m["bytes"][3])
            icao = icao if address is None else int(address[k])
            print(f"{t:14.6f} {icao:06X} {f['latitude']:10.5f} {f['longitude']:11.5f} {f['height_m']:8.0f} "
                  f"{f['residual_rms_m']:8.1f} {f['hdop']:6.1f} {int(f['n_used']):3d}")
    print(f"# {int(hdr['n_messages'])} messages, {int(hdr['n_attempted'])} attempted, {int(hdr['n_valid'])} valid",
          file=sys.stderr)
    return 0


if __name__ == "__main__":
    sys.exit(main())
