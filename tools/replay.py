#!/usr/bin/env python3
"""Replay an IQ capture through the GPU path and print what `air_rs adsb -p FILE -m stream` prints
(reference: src/main.rs:19-23 -> launch_adsb, src/adsb.rs:126-173; text format src/adsb/packet.rs:77-99).

  tools/replay.py capture.c16                 # the reference's format (utils.rs:22-43), reference semantics
  tools/replay.py capture.bin --format u8     # raw rtl_sdr capture (unsigned bytes)
  tools/replay.py capture.c16 --carry --tail  # also decode frames straddling buffers and the last chunk
  tools/replay.py capture.c16 --aircraft      # the final aircraft table instead (tui.rs:65-95, Velocity filled)
  tools/replay.py capture.c16 --web           # what the web thread broadcasts instead: one JSON line per packet
  tools/replay.py capture.c16 --levels        # signal and noise power of every packet instead, tab-separated
  tools/replay.py capture.c16 --aircraft --levels   # the aircraft table with two more columns: RSSI and SNR
  tools/replay.py capture.c16 --aircraft --site 51.5,-0.1      # ... with five more: each aircraft's own fix from the site
  tools/replay.py capture.c16 --beast out.bin # also write every packet as Beast binary (readsb / dump1090 / tar1090 input)
  tools/replay.py capture.c16 --avr out.txt   # ... as AVR text, one "*...;" line per packet; --mlat: "@" + timestamp + ...
  tools/replay.py out.bin --beast-in          # FILE is a Beast capture (a receiver's TCP stream) instead of IQ
  tools/replay.py out.txt --avr-in            # ... an AVR text capture, "*" and "@" lines alike
  tools/replay.py out.txt --avr-in --modes --commb   # one line per frame; DF20/21 lines with their Comm-B register
  tools/replay.py out.txt --avr-in --es       # one line per DF17/18 frame: what it says about the aircraft's status
  tools/replay.py capture.bin --replies --modes      # the packets and the Mode S replies found in the samples, one list
  tools/replay.py capture.bin --replies --beast out.bin --levels   # ... sent out again, short frames as Beast '2'

Everything below the argument parsing is one call through the C ABI (adsb_replay_file, include/adsb_host.h).
The "Processed Time" line carries no value (the reference prints the wall clock there).  With --aircraft, the frames
go through one device track table (2 MSPS, one update) and the table is printed tab-separated with the columns of
the reference's TUI; its Velocity column, always "n/a" there, holds the last airborne-velocity message's speed.
With --web, the frames go through one device track table with a summaries reserve, one update per buffer, and every
frame's summary is printed as one JSON line: the reference's serialisation of AircraftSummary (aircraft.rs:14-23,
cpr.rs:10-16, camelCase), which its web thread sends for every packet (web.rs:117-128).  lastContact is whole seconds
of frame time (0 when the aircraft has had no position message): the reference stamps the wall clock there.  Floats
are printed with Python's shortest round-trip repr.  With --levels, one line per packet: offset, ICAO (hex), signal
dBFS, noise dBFS, their difference, weak bits -- the mean power of the packet's 116 pulse samples and of its 124 quiet
samples against a full-scale sample, one decimal, "-inf" for a sum of zero; computed on the device over the capture in
device memory (adsb_levels_of), in overlapping pieces if the capture is large.  With --aircraft --levels, the table's
update also merges every frame's level record (the host mirror's, adsb_host_frame_levels) into the aircraft's level
record on the device, and two columns are appended: RSSI, the aircraft's mean signal power in dBFS over its 116 x
n_levels pulse samples, and SNR, that minus its mean noise power in dBFS over 124 x n_levels quiet samples, one decimal,
"n/a" in both for an aircraft without a counted frame; --aircraft alone prints what it always printed.  With --aircraft
--site LAT,LON[,RANGE_NM] (degrees, nautical miles; default range 180) the table gets a fixes reserve with that receiver
site and five columns are appended (after RSSI and SNR if both are asked for): FixLat and FixLon, the position of the
aircraft's newest position message decoded on its own against the site (six decimals; this also covers surface
messages and aircraft heard with one CPR format only, which Latitude and Longitude never show), Range in nautical miles
and Bearing in degrees from the site (one decimal), and GS, a surface message's ground speed in knots (one decimal);
"n/a" for a missing value (write a negative latitude as --site=-33.9,151.2).  With --beast FILE / --avr FILE the
whole capture's packets are also written to FILE as one stream, encoded on the device (adsb_wire_of): Beast binary with
the 12 MHz timestamp 6 x offset + N (--tick-bias N, default 0: the first preamble sample) and the signal byte from the
packets' level records, or AVR text ("*" lines; with --mlat "@" lines that carry the timestamp).  Offsets are positions
in the whole capture, so the timestamps run on across chunks.  With --beast-in / --avr-in the positional file holds
Beast binary or AVR text instead of samples: it is parsed on the device (adsb_wire_in_of) in 64 KiB chunks, the unparsed
tail of each carried into the next by `consumed`, frame offsets = (timestamp - N) / 6 (--tick-bias N), and everything
that prints from a frame list works on it: the stream text, --aircraft (with --levels: RSSI from the Beast signal
bytes), --web, --beast, --avr.  --levels alone needs the samples.  With --modes (and --beast-in / --avr-in) the 56-bit frames are
parsed too (ADSB_WIRE_IN_SHORT), every frame gets its address on the device (adsb_modes_of, the known addresses carried from
chunk to chunk), and one line per frame is printed instead: time in seconds, DF, kind (SELF, KNOWN, UNKNOWN, PARITY,
UNSUPPORTED), address, altitude in feet, squawk and callsign, "-" for a missing value.  With --modes --aircraft the frames
and their Mode S records go through one device track table with a modes reserve (adsb_track_table_update_modes: keyed by
the resolved address, so aircraft that only answer interrogations have a row; frames without an aircraft's address touch
nothing) and the table is printed with five more columns: Alt(S), Squawk and Call(S) from the aircraft's newest replies
that carry them, Replies, and S, which is "S" for an aircraft that has sent no DF17/18 frame.  With --modes --commb
every DF20/21 line also ends with the Comm-B register its MB field carries, inferred on the device from the 56 bits
(adsb_commb_of, on the list where wire input left it): "BDS4,0 mcp=3008ft fms=3008ft baro=1020.0mb", the values whose
status bit is set in feet, mb, degrees, kt, Mach, degrees per second and ft/min; for BDS 1,7 the registers the
transponder reports; "?" and the candidates ("?5,0|6,0") where more than one register fits, "-" where none does or MB
is empty.  With --es (on samples, --beast-in and --avr-in alike) the frame list goes through the extended squitter
status stage (adsb_es_of) and one line per DF17/18 frame is printed instead: time in seconds, DF, the address in the
frame, and the state with its values: "CATEGORY A0", "POSITION tc=11 nic_b=0 rc=185.2m", "VELOCITY st=1 nac_v=0 ifr",
"EMERGENCY state=0 squawk=6513", "ACAS_RA ara=... rac=. rat=. mte=. tti=. tid=.......", "TARGET_STATE alt=16992ft(mcp)
baro=1012.8mb hdg=66.8 nac_p=9 nic_baro=1 sil=3 modes=autopilot,vnav,lnav tcas", "OPERATIONAL st=0 v2 cc=2300 om=0300
nic_a=0 nac_p=9 sil=3 nic_baro=1 sil_supp=0 sda=3 gva=2", "RESERVED tc=23 st=0", "FOREIGN"; a value the frame does not hold is left
out.  The stage does not check parity: the frames of a Beast or AVR capture are read as they stand.
With --es --aircraft (samples, --beast-in, --avr-in, with --modes or without) the table takes those records too
(adsb_track_table_update_es) and eight columns are appended: Ver (the aircraft's ADS-B version), NIC and Rc in metres of
its newest position message, resolved with the version and the NIC supplements the aircraft sent in its operational
status messages (a "?" behind both where no version was known when that message was heard: Rc is then what the type
code alone gives), NACp and SIL of the newest operational status or target state message, Emerg and Squawk(ES) of the
newest TC 28 message, and SelAlt, the selected altitude in feet.
With --replies (on samples) the whole capture goes to device memory once: the demodulator's launch gives the DF17 list as
ever, the replies scan (adsb_replies_of: DF11, DF18 and the address/parity formats DF0/4/5/16/20/21, by a preamble and
parity rule of its own on sample power) gives a second list from the same samples, and the two are merged on the device
(adsb_merge_lists_of).  One line per frame: time in seconds, offset, "demod" or "replies", DF and the message in hex.
With --replies --modes the merged list goes through adsb_modes_of and --modes' lines are printed; with --replies --modes
--aircraft the table keyed by the resolved addresses.  No chunking here: offsets are positions in the capture.
With --replies --beast FILE / --avr FILE [--mlat] the merged list is also written as one stream with ADSB_WIRE_SHORT:
56-bit frames leave as Beast '2' frames or 14-digit lines, the Beast signal bytes from the list's level records by frame
length (adsb_levels_modes_of on the capture in device memory).  With --replies --levels one line per frame instead:
offset, DF, signal dBFS, noise dBFS, their difference, weak bits; a 56-bit frame's over 60 pulse and 68 quiet samples.
The TEXT has not been compared with a Rust build's (there is no
Rust toolchain); only the values are checked, against the oracle."""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import air_rs_amd as A  # noqa: E402
from air_rs_amd import _lib as L  # noqa: E402


SECONDS_PER_SAMPLE = 0.5e-6  # 2 MSPS


def mean_dbfs(st, total, n_samples):
    """adsb_level_dbfs in Python floats (its n_samples is 32 bits; an aircraft's 116 x n_levels need not fit)."""
    full_scale = 32768.0 if st == A.ADSB_SAMPLE_I8 else 2147483648.0
    return -math.inf if total == 0 else 10.0 * math.log10(float(total) / float(n_samples) / full_scale)


def level_columns(st, lv):
    """RSSI and SNR of one AIRCRAFT_LEVEL_DTYPE record."""
    n = int(lv["n_levels"])
    if n == 0:
        return ["n/a", "n/a"]
    sig = mean_dbfs(st, int(lv["signal_total"]), A.LEVEL_PULSE_SAMPLES * n)
    noise = mean_dbfs(st, int(lv["noise_total"]), A.LEVEL_QUIET_SAMPLES * n)
    return [f"{sig:.1f}", f"{sig - noise:.1f}"]


def parse_site(text):
    """LAT,LON[,RANGE_NM] -> (latitude, longitude, max_range_nm)"""
    parts = [float(x) for x in text.split(",")]
    if len(parts) not in (2, 3):
        raise argparse.ArgumentTypeError("expected LAT,LON[,RANGE_NM]")
    return (parts[0], parts[1], parts[2] if len(parts) == 3 else 180.0)


def fix_columns(fx):
    """FixLat, FixLon, Range, Bearing and GS of one FIX_DTYPE record."""
    if not fx["flags"] & A.ADSB_FIX_VALID:
        return ["n/a"] * 5
    return [f"{float(fx['latitude']):.6f}", f"{float(fx['longitude']):.6f}", f"{float(fx['range_nm']):.1f}",
            f"{float(fx['bearing_deg']):.1f}",
            f"{float(fx['ground_speed_kt']):.1f}" if fx["flags"] & A.ADSB_FIX_SPEED else "n/a"]


def modes_columns(s):
    """Alt(S), Squawk, Call(S), Replies and S of one AIRCRAFT_MODES_DTYPE record."""
    flags = int(s["flags"])
    return [f"{int(s['altitude_ft'])}" if flags & A.ADSB_TRACK_MODES_ALT else "n/a",
            f"{int(s['squawk']):04d}" if flags & A.ADSB_TRACK_MODES_SQUAWK else "n/a",
            (s["callsign"].decode("ascii", "replace").replace("_", " ").strip() or "n/a")
            if flags & A.ADSB_TRACK_MODES_CALLSIGN else "n/a",
            f"{int(s['n_replies'])}", "" if flags & A.ADSB_TRACK_MODES_SQUITTER else "S"]


def aircraft_table(d, frames, n_samples, st=None, frame_levels=None, site=None, modes=None, commb=None, es=None):
    """The capture's final aircraft table as tab-separated text: tui.rs:95's columns, rows by age (tui.rs:69), then
    ICAO.  Age = whole seconds from each aircraft's last frame to the end of the capture.  frame_levels (one
    LEVEL_DTYPE record per frame, with st the sample type): also the columns RSSI and SNR.  site ((latitude, longitude,
    max_range_nm)): also FixLat, FixLon, Range, Bearing and GS.  modes (one MODES_DTYPE record per frame): the table is
    keyed by the records' addresses (update_modes); also Alt(S), Squawk, Call(S), Replies and S.  commb (with modes: one
    COMMB_DTYPE record per frame): the table also keeps the aircraft's Comm-B registers (update_commb) and settles a reply
    that reads as 5,0 and as 6,0 from the aircraft's ADS-B velocity; also SelAlt, QNH, GS/Trk(B), Hdg, IAS and Mach, with
    a "*" behind a value from a settled reply.  es (one ES_DTYPE record per frame): the table also keeps the aircraft's
    extended squitter status (update_es) and resolves NIC and Rc of every position message with the aircraft's version and
    NIC supplements; also Ver, NIC, Rc, NACp, SIL, Emerg, Squawk(ES) and SelAlt, with a "?" behind NIC and Rc of an
    aircraft whose version was not known when its newest position was heard (Rc is then the type code's own)."""
    with A.TrackTable(d, max_frames=max(len(frames), 1), seconds_per_sample=SECONDS_PER_SAMPLE) as t:
        if site is not None:
            t.fixes_reserve(site)
        if modes is not None:
            t.modes_reserve()
        more = {}
        if commb is not None:
            t.commb_reserve()
            more["commb"] = commb
        if es is not None:
            t.es_reserve()
            more["es"] = es
        if frame_levels is None:
            t.update(frames, modes=modes, **more)
        else:
            t.levels_reserve()
            t.update(frames, levels=frame_levels, modes=modes, **more)
        recs, _ = t.aircraft()
        vel, heard = t.velocity(), t.last_heard()
        sides = [None] * len(recs) if modes is None else t.modes()
        levels = [None] * len(recs) if frame_levels is None else t.levels()
        fixes = [None] * len(recs) if site is None else t.fixes()
        registers = [None] * len(recs) if commb is None else A.aircraft_commb_columns(t.commb())
        status = [None] * len(recs)
        if es is not None:
            status = A.aircraft_es_columns(t.es())
    now = n_samples * SECONDS_PER_SAMPLE
    rows = []
    for rec, v, lh, lv, fx, side, reg, stat in zip(recs, vel, heard, levels, fixes, sides, registers, status):
        pos, age = bool(rec["has_position"]), int(now - lh)
        rows.append((age, int(rec["icao"]), "\t".join([
            f"{int(rec['icao']):x}",
            rec["callsign"].decode("latin-1"),                       # S8: trailing NULs already stripped
            f"{int(rec['altitude'])}",
            f"{float(rec['latitude']):.6f}" if pos else "n/a",
            f"{float(rec['longitude']):.6f}" if pos else "n/a",
            f"{float(v['speed_kt']):.0f}" if v["flags"] & A.ADSB_VELOCITY_SPEED else "n/a",
            f"{age}"] + ([] if lv is None else level_columns(st, lv)) + ([] if fx is None else fix_columns(fx))
            + ([] if side is None else modes_columns(side)) + ([] if reg is None else reg) + ([] if stat is None else stat))))
    rows.sort(key=lambda r: (r[0], r[1]))
    head = "ICAO\tCallsign\tAltitude\tLatitude\tLongitude\tVelocity\tAge" + ("" if frame_levels is None else "\tRSSI\tSNR")
    head += "" if site is None else "\tFixLat\tFixLon\tRange\tBearing\tGS"
    head += "" if modes is None else "\tAlt(S)\tSquawk\tCall(S)\tReplies\tS"
    head += "" if commb is None else "\t" + "\t".join(A.AIRCRAFT_COMMB_COLUMNS)
    head += "" if es is None else "\t" + "\t".join(A.AIRCRAFT_ES_COLUMNS)
    return head + "\n" + "".join(r[2] + "\n" for r in rows)


def summary_json(rec):
    """One summaries() record as the reference's AircraftSummary JSON (key order of the struct)."""
    contact = float(rec["last_contact"])
    return json.dumps({
        "icao": int(rec["icao"]),
        "callsign": rec["callsign"].decode("latin-1"),           # S8: trailing NULs already stripped
        "altitude": int(rec["altitude"]),
        "geoPosition": {"latitude": float(rec["latitude"]), "longitude": float(rec["longitude"])}
        if rec["has_position"] else None,
        "lastContact": 0 if math.isnan(contact) else int(contact)}, separators=(",", ":"))


def web_stream(d, frames, chunk):
    """One JSON line per frame: the frame's aircraft right after it, one table update per buffer of `chunk` samples."""
    lines = []
    with A.TrackTable(d, max_frames=max(len(frames), 1), seconds_per_sample=SECONDS_PER_SAMPLE) as t:
        t.summaries_reserve()
        a = 0
        while a < len(frames):
            buf = int(frames[a]["offset"]) // chunk
            b = a
            while b < len(frames) and int(frames[b]["offset"]) // chunk == buf:
                b += 1
            t.update(frames[a:b])
            lines.extend(summary_json(rec) for rec in t.summaries())
            a = b
    return "".join(line + "\n" for line in lines)


LEVELS_PIECE = 1 << 26  # samples of the capture in device memory at a time (--levels)


def read_capture(path, fmt):
    """The capture as the library reads it: (n, 2) int16 for .c16, int8 (x - 128) for raw rtl_sdr bytes."""
    import numpy as np
    if fmt == "c16":
        return np.fromfile(path, dtype="<i2").reshape(-1, 2)
    return (np.fromfile(path, dtype=np.uint8) ^ 0x80).view(np.int8).reshape(-1, 2)


def level_lines(d, st, frames, iq, piece=LEVELS_PIECE):
    """One tab-separated line per frame: offset, ICAO, signal dBFS, noise dBFS, signal - noise, weak bits.  The
    capture goes to device memory piece by piece; neighbouring pieces overlap by 239 samples, so every frame's 240
    samples lie in the piece that owns its offset."""
    import numpy as np
    import torch
    lines, step = [], piece - (A.WINDOW - 1)
    offsets = frames["offset"].astype(np.int64)
    for start in range(0, max(len(iq) - (A.WINDOW - 1), 1), step):
        mine = frames[(offsets >= start) & (offsets < start + step)]
        if not len(mine):
            continue
        part = torch.from_numpy(np.ascontiguousarray(iq[start:start + piece])).to(f"cuda:{d.device}")
        levels = d.levels_of(part.data_ptr(), part.shape[0], mine, first_sample=start)
        del part
        for f, lv in zip(mine, levels):
            sig = A.level_dbfs(st, lv["signal_sum"], A.LEVEL_PULSE_SAMPLES)
            noise = A.level_dbfs(st, lv["noise_sum"], A.LEVEL_QUIET_SAMPLES)
            icao = int(f["bytes"][1]) << 16 | int(f["bytes"][2]) << 8 | int(f["bytes"][3])
            lines.append(f"{int(f['offset'])}\t{icao:x}\t{sig:.1f}\t{noise:.1f}\t{sig - noise:.1f}\t{int(lv['weak_bits'])}")
    return "".join(line + "\n" for line in lines)


WIRE_IN_CHUNK = 1 << 16  # bytes of a Beast / AVR capture parsed at a time


COMMB_1_7 = ("0,5 0,6 0,7 0,8 0,9 0,A 2,0 2,1 4,0 4,1 4,2 4,3 4,4 4,5 4,8 5,0 5,1 5,2 5,3 5,4 5,5 5,6 5,F 6,0").split()
COMMB_NAMES = {0x10: "1,0", 0x17: "1,7", 0x20: "2,0", 0x30: "3,0", 0x40: "4,0", 0x50: "5,0", 0x60: "6,0"}
# --commb, registers with status bits: (label, key of commb_physical or None for the raw value, format) per value
COMMB_FIELDS = {
    0x40: (("mcp", "mcp_altitude_ft", "{:.0f}ft"), ("fms", "fms_altitude_ft", "{:.0f}ft"), ("baro", "baro_setting_mb", "{:.1f}mb"),
           ("mode", None, "{}"), ("source", None, "{}")),
    0x50: (("roll", "roll_deg", "{:.2f}"), ("track", "true_track_deg", "{:.2f}"), ("gs", "ground_speed_kt", "{:.0f}kt"),
           ("rate", "track_rate_deg_s", "{:.3f}"), ("tas", "true_airspeed_kt", "{:.0f}kt")),
    0x60: (("hdg", "magnetic_heading_deg", "{:.2f}"), ("ias", "ias_kt", "{:.0f}kt"), ("mach", "mach", "{:.3f}"),
           ("baro", "baro_rate_ft_min", "{:.0f}ft/min"), ("inertial", "inertial_rate_ft_min", "{:.0f}ft/min")),
}


def commb_text(c):
    """--commb: what one COMMB_DTYPE record adds to a DF20/21 line: "BDSr,n" and the register's values (those whose
    status bit is set, in physical units), "?" and the candidates for AMBIGUOUS, "-" for an empty MB or no candidate."""
    state = int(c["state"])
    if state == A.ADSB_COMMB_AMBIGUOUS:
        return "?" + "|".join(name for k, name in enumerate(COMMB_NAMES.values()) if int(c["candidates"]) >> k & 1)
    if state != A.ADSB_COMMB_ONE:
        return "-"
    bds, value, word = int(c["bds"]), [int(v) for v in c["value"]], int(c["word"])
    parts = ["BDS" + COMMB_NAMES[bds]]
    if bds in COMMB_FIELDS:
        phys = A.commb_physical(c)
        for k, (label, key, fmt) in enumerate(COMMB_FIELDS[bds]):
            if int(c["status"]) >> k & 1:
                parts.append(label + "=" + fmt.format(value[k] if key is None else float(phys[key][0])))
    elif bds == 0x17:
        parts += [name for k, name in enumerate(COMMB_1_7) if word >> (27 - k) & 1]
    elif bds == 0x10:
        parts += [f"version={value[0]}", f"ovc={value[1]}"]
    elif bds == 0x30:
        parts += [f"ara={value[0]:04X}", f"rac={value[1]:X}", f"rat_mte={value[2]}", f"tti={value[3]}", f"tid={value[4]:07X}"]
    return " ".join(parts)


ES_MODE_FLAGS = (("autopilot", A.ADSB_ES_AUTOPILOT), ("vnav", A.ADSB_ES_VNAV), ("alt_hold", A.ADSB_ES_ALT_HOLD),
                 ("approach", A.ADSB_ES_APPROACH), ("lnav", A.ADSB_ES_LNAV))
# --es, OPERATIONAL: (label, field, present bit) in the order printed
ES_OPERATIONAL = (("nic_a", "nic_a", A.ADSB_ES_HAS_NIC_A), ("nac_p", "nac_p", A.ADSB_ES_HAS_NAC_P), ("sil", "sil", A.ADSB_ES_HAS_SIL),
                  ("nic_baro", "nic_baro", A.ADSB_ES_HAS_NIC_BARO), ("lw", "length_width", A.ADSB_ES_HAS_LENGTH_WIDTH),
                  ("sil_supp", "sil_supplement", A.ADSB_ES_HAS_SIL_SUPPLEMENT), ("sda", "sda", A.ADSB_ES_HAS_SDA),
                  ("gva", "gva", A.ADSB_ES_HAS_GVA), ("nic_c", "nic_c", A.ADSB_ES_HAS_NIC_C), ("nac_v", "nac_v", A.ADSB_ES_HAS_NAC_V))


def es_text(r):
    """--es: the state of one ES_DTYPE record and the values it holds, in physical units where es_physical has one."""
    state, has, flags = int(r["state"]), int(r["present"]), int(r["flags"])
    parts, phys = [A.ES_STATES[state]], A.es_physical(r)
    if state == A.ADSB_ES_CATEGORY:
        parts.append(f"{int(r['category']):02X}")
    elif state == A.ADSB_ES_POSITION:
        parts.append(f"tc={int(r['type_code'])}")
        if has & A.ADSB_ES_HAS_NIC_B:
            parts.append(f"nic_b={int(r['nic_b'])}")
        if has & A.ADSB_ES_HAS_RC:
            parts.append(f"rc={float(phys['rc_m'][0]):.1f}m")
    elif state == A.ADSB_ES_VELOCITY:
        parts += [f"st={int(r['subtype'])}", f"nac_v={int(r['nac_v'])}"]
        parts += [name for name, bit in (("intent", A.ADSB_ES_INTENT_CHANGE), ("ifr", A.ADSB_ES_IFR)) if flags & bit]
    elif state == A.ADSB_ES_EMERGENCY:
        parts += [f"state={int(r['emergency'])}", f"squawk={int(r['half'][0]):04d}"]
    elif state == A.ADSB_ES_ACAS_RA:
        bits = int(r["value"]) << 16 | int(r["half"][0])             # ARA 14, RAC 4, RAT 1, MTE 1, TTI 2, TID 26
        parts += [f"ara={bits >> 34:04X}", f"rac={bits >> 30 & 15:X}", f"rat={bits >> 29 & 1}", f"mte={bits >> 28 & 1}",
                  f"tti={bits >> 26 & 3}", f"tid={bits & 0x3FFFFFF:07X}"]
    elif state == A.ADSB_ES_TARGET_STATE:
        if has & A.ADSB_ES_HAS_SELECTED_ALT:
            parts.append(f"alt={float(phys['selected_altitude_ft'][0]):.0f}ft({'fms' if flags & A.ADSB_ES_ALT_FMS else 'mcp'})")
        if has & A.ADSB_ES_HAS_BARO:
            parts.append(f"baro={float(phys['baro_setting_mb'][0]):.1f}mb")
        if has & A.ADSB_ES_HAS_HEADING:
            parts.append(f"hdg={float(phys['selected_heading_deg'][0]):.1f}")
        parts += [f"nac_p={int(r['nac_p'])}", f"nic_baro={int(r['nic_baro'])}", f"sil={int(r['sil'])}"]
        if int(r["sil_supplement"]):
            parts.append("sil_supp=1")
        if has & A.ADSB_ES_HAS_MODES:
            parts.append("modes=" + (",".join(name for name, bit in ES_MODE_FLAGS if flags & bit) or "none"))
        if flags & A.ADSB_ES_TCAS:
            parts.append("tcas")
    elif state == A.ADSB_ES_OPERATIONAL:
        parts += [f"st={int(r['subtype'])}", f"v{int(r['version'])}"]
        if has & A.ADSB_ES_HAS_CC_OM:
            parts += [f"cc={int(r['half'][0]):04X}", f"om={int(r['half'][1]):04X}"]
        parts += [f"{label}={int(r[field])}" for label, field, bit in ES_OPERATIONAL if has & bit]
        parts += [name for name, bit, on in (("hrd", A.ADSB_ES_HAS_HRD, A.ADSB_ES_HRD),
                                             ("heading", A.ADSB_ES_HAS_TRACK_HEADING, A.ADSB_ES_TRACK_HEADING)) if has & bit and flags & on]
    elif state == A.ADSB_ES_RESERVED:
        parts += [f"tc={int(r['type_code'])}", f"st={int(r['subtype'])}"]
    return " ".join(parts)


def es_lines(frames, recs):
    """--es: one line per DF17/18 frame from its ES_DTYPE record."""
    out = []
    for f, r in zip(frames, recs):
        if int(r["state"]) != A.ADSB_ES_NOT_ES:
            b = f["bytes"]
            out.append(f"{int(f['offset']) * SECONDS_PER_SAMPLE:.6f} DF{int(b[0]) >> 3} {int(b[1]) << 16 | int(b[2]) << 8 | int(b[3]):06X} "
                       f"{es_text(r)}\n")
    return "".join(out)


def modes_lines(frames, recs, commb=None):
    """--modes: one line per frame from its MODES_DTYPE record; commb (one COMMB_DTYPE record per frame): the DF20/21
    lines end with commb_text()."""
    out = []
    for j, (f, r) in enumerate(zip(frames, recs)):
        flags = int(r["flags"])
        alt = f"{int(r['altitude_ft'])}" if flags & A.ADSB_MODES_ALT else "-"
        squawk = f"{int(r['squawk']):04d}" if flags & A.ADSB_MODES_SQUAWK else "-"
        call = r["callsign"].decode("ascii", "replace").replace("_", " ").strip() if flags & A.ADSB_MODES_CALLSIGN else "-"
        addr = f"{int(r['address']):06X}" if int(r["kind"]) <= A.ADSB_MODES_UNKNOWN else "-"
        more = "" if commb is None or int(r["df"]) not in (20, 21) else " " + commb_text(commb[j])
        out.append(f"{int(f['offset']) * SECONDS_PER_SAMPLE:.6f} DF{int(r['df'])} {A.MODES_KINDS[int(r['kind'])]} {addr} "
                   f"{alt} {squawk} {call or '-'}{more}\n")
    return "".join(out)


def replies_lines(frames, src):
    """--replies: one line per frame of the merged list: time in seconds, offset, where it comes from ("demod": the
    demodulator's DF17 list, "replies": the replies scan), DF, and the message in hex, 14 digits for a 56-bit frame."""
    out = []
    for f, s in zip(frames, src):
        df = int(f["bytes"][0]) >> 3
        msg = f["bytes"][:7 if df < 16 else 14].tobytes().hex().upper()
        out.append(f"{int(f['offset']) * SECONDS_PER_SAMPLE:.6f} {int(f['offset'])} "
                   f"{'replies' if int(s) & A.ADSB_MERGE_FROM_B else 'demod'} DF{df} {msg}\n")
    return "".join(out)


def replies_level_lines(st, frames, levels):
    """--replies --levels: one tab-separated line per frame of the merged list: offset, DF, signal dBFS, noise dBFS,
    signal - noise, weak bits.  A 56-bit frame's record (ADSB_LEVEL_SHORT) is over 60 pulse and 68 quiet samples, a
    112-bit frame's over 116 and 124; a frame whose window is not inside the capture gets "n/a"."""
    out = []
    for f, lv in zip(frames, levels):
        head = f"{int(f['offset'])}\tDF{int(f['bytes'][0]) >> 3}"
        flags = int(lv["flags"])
        if not flags & A.ADSB_LEVEL_VALID:
            out.append(head + "\tn/a\tn/a\tn/a\tn/a\n")
            continue
        short = bool(flags & A.ADSB_LEVEL_SHORT)
        sig = A.level_dbfs(st, lv["signal_sum"], A.LEVEL_SHORT_PULSE_SAMPLES if short else A.LEVEL_PULSE_SAMPLES)
        noise = A.level_dbfs(st, lv["noise_sum"], A.LEVEL_SHORT_QUIET_SAMPLES if short else A.LEVEL_QUIET_SAMPLES)
        out.append(f"{head}\t{sig:.1f}\t{noise:.1f}\t{sig - noise:.1f}\t{int(lv['weak_bits'])}\n")
    return "".join(out)


def replies_run(device, st, iq, levels=None):
    """--replies: the demodulator's launch and the replies scan over the whole capture in device memory, merged on the
    device -> (the context, which the caller closes; merged frames; src; the level records or None).  levels: "device"
    computes the merged list's level records by frame length (adsb_levels_modes_of on the capture where it lies) and
    leaves them on the device, d.levels_modes_device(); "host" also returns them; None: no records."""
    import numpy as np
    import torch
    n = len(iq)
    d = A.AdsbDemod(device=device, sample_type=st, max_samples=max(n, A.WINDOW), max_out=max(n // 100, 1 << 16), host_staging=False)
    dev = torch.from_numpy(np.ascontiguousarray(iq)).to(f"cuda:{device}")
    found = np.zeros(0, dtype=A.FRAME_DTYPE)
    if n >= A.WINDOW:
        d.demod_device_async(dev.data_ptr(), n)
        found = d.fetch()[0]
    replies, _, hdr = d.replies_of(dev.data_ptr(), n_samples=n)
    if int(hdr["flags"]) & A.ADSB_FLAG_TRUNCATED:
        print(f"replies scan: {int(hdr['total_found'])} frames found, {len(replies)} kept", file=sys.stderr)
    frames, src, _ = d.merge_lists(found, [len(found)], replies, [len(replies)])
    records = d.levels_modes_of(dev.data_ptr(), n, frames, fetch=levels == "host") if levels else None
    del dev
    return d, frames, src, records


def read_wire(d, path, wire_format, tick_bias, chunk=WIRE_IN_CHUNK, modes=False, commb=False):
    """--beast-in / --avr-in: (frames, their level records) of a Beast or AVR capture, parsed on the device chunk by
    chunk; what a chunk leaves unparsed (an incomplete last frame) goes in front of the next.  modes: short frames too,
    and (frames, their MODES_DTYPE records), each chunk resolved where it lies with the known addresses of the chunks
    before it.  commb (with modes): (frames, records, their COMMB_DTYPE records), from the same device list
    (adsb_commb_of)."""
    import numpy as np
    frames, levels, tail = [np.zeros(0, dtype=A.FRAME_DTYPE)], [np.zeros(0, dtype=A.LEVEL_DTYPE)], b""
    if modes:
        recs, known = [np.zeros(0, dtype=A.MODES_DTYPE)], np.zeros(0, dtype=np.uint32)
        regs = [np.zeros(0, dtype=A.COMMB_DTYPE)]
        with open(path, "rb") as fh:
            while True:
                new = fh.read(chunk)
                if not new:
                    break
                got = d.wire_in_of(tail + new, format=wire_format, tick_bias=tick_bias, filter="short")
                rec, known = d.modes_of((d.wire_in_device()[0], len(got.frames)), None, known)[:2]
                if commb:
                    regs.append(d.commb_of((d.wire_in_device()[0], len(got.frames)))[0])
                frames.append(got.frames)
                recs.append(rec)
                tail = (tail + new)[int(got.consumed[0]):]
        if commb:
            return np.concatenate(frames), np.concatenate(recs), np.concatenate(regs)
        return np.concatenate(frames), np.concatenate(recs)
    with open(path, "rb") as fh:
        while True:
            new = fh.read(chunk)
            if not new:
                break
            got = d.wire_in_of(tail + new, format=wire_format, tick_bias=tick_bias, levels=True)
            frames.append(got.frames)
            levels.append(got.levels)
            tail = (tail + new)[int(got.consumed[0]):]
    return np.concatenate(frames), np.concatenate(levels)


def stream_text(frames):
    """What the stream thread prints for a frame list (adsb.rs:156-158)."""
    return "".join("\n" + A.packet_display(f["bytes"].tobytes()) + "\n" for f in frames)


def write_wire(d, frames, a, fmt, levels=None):
    """--beast / --avr: the capture's frames as one stream, encoded on the device."""
    if a.beast:
        levels = A.host_frame_levels(read_capture(a.file, fmt), frames) if levels is None else levels
        with open(a.beast, "wb") as fh:
            fh.write(d.wire_of(frames, levels, format="beast", tick_bias=a.tick_bias)[0])
    if a.avr:
        with open(a.avr, "wb") as fh:
            fh.write(d.wire_of(frames, None, format="avr_mlat" if a.mlat else "avr", tick_bias=a.tick_bias)[0])


def write_replies_wire(d, frames, a):
    """--replies --beast / --avr: the merged list as one stream with ADSB_WIRE_SHORT, so that 56-bit frames leave as
    Beast '2' frames or 14-digit lines; the Beast signal bytes from the level records replies_run left on the device."""
    if a.beast:
        with open(a.beast, "wb") as fh:
            fh.write(d.wire_of(frames, d.levels_modes_device() if len(frames) else None, format="beast",
                               tick_bias=a.tick_bias, short=True)[0])
    if a.avr:
        with open(a.avr, "wb") as fh:
            fh.write(d.wire_of(frames, None, format="avr_mlat" if a.mlat else "avr", tick_bias=a.tick_bias, short=True)[0])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("file")
    ap.add_argument("--format", choices=["c16", "u8"], default=None, help="default: by extension (.c16 -> c16, else u8)")
    ap.add_argument("--chunk", type=int, default=20000, help="samples per buffer (adsb.rs:77-79: 20000)")
    ap.add_argument("--carry", action="store_true", help="carry the last 240 samples over (not reference behaviour)")
    ap.add_argument("--tail", action="store_true", help="also send the last chunk (not reference behaviour)")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--summary", action="store_true", help="print counts to stderr")
    ap.add_argument("--aircraft", action="store_true", help="print the final aircraft table instead of the stream text")
    ap.add_argument("--web", action="store_true", help="print one AircraftSummary JSON line per packet instead")
    ap.add_argument("--levels", action="store_true", help="print signal and noise power of every packet instead; with --aircraft: two more columns, RSSI and SNR")
    ap.add_argument("--site", type=parse_site, default=None, metavar="LAT,LON[,RANGE_NM]",
                    help="with --aircraft: the receiver's position; five more columns: FixLat, FixLon, Range, Bearing, GS")
    ap.add_argument("--beast", metavar="FILE", help="also write the packets to FILE as Beast binary")
    ap.add_argument("--avr", metavar="FILE", help="also write the packets to FILE as AVR text")
    ap.add_argument("--mlat", action="store_true", help="with --avr: the '@' form, which carries the 12 MHz timestamp")
    ap.add_argument("--beast-in", action="store_true", help="FILE is a Beast binary capture instead of IQ")
    ap.add_argument("--avr-in", action="store_true", help="FILE is an AVR text capture instead of IQ")
    ap.add_argument("--modes", action="store_true",
                    help="with --beast-in / --avr-in: short frames too; print DF, kind, address, altitude, squawk, callsign per "
                         "frame, or with --aircraft the table keyed by those addresses")
    ap.add_argument("--commb", action="store_true",
                    help="with --modes: every DF20/21 line also gets the Comm-B register inferred from its MB field and its "
                         "values; with --modes --aircraft: six more columns from the aircraft's Comm-B registers")
    ap.add_argument("--es", action="store_true",
                    help="print one line per DF17/18 frame instead: its extended squitter status (category, emergency, target "
                         "state, operational status, NACv, NIC supplement B, stand-alone Rc); with --aircraft: eight more "
                         "columns from the aircraft's extended squitter status, NIC and Rc resolved per aircraft")
    ap.add_argument("--replies", action="store_true",
                    help="on samples: also run the replies scan (DF11, DF18, DF0/4/5/16/20/21 from the samples), merge its list "
                         "with the packets and print one line per frame; with --modes: address and kind per frame; with "
                         "--modes --aircraft: the table keyed by those addresses")
    ap.add_argument("--tick-bias", type=int, default=0, metavar="N", help="added to every timestamp (12 MHz ticks, < 2^48)")
    a = ap.parse_args()
    if a.mlat and not a.avr:
        ap.error("--mlat needs --avr")
    if not 0 <= a.tick_bias < 1 << 48:
        ap.error("--tick-bias is 0 .. 2^48 - 1")
    if a.site is not None and not a.aircraft:
        ap.error("--site needs --aircraft")
    if a.beast_in and a.avr_in:
        ap.error("--beast-in and --avr-in exclude each other")
    wire_in = "beast" if a.beast_in else "avr" if a.avr_in else None
    if a.replies and (wire_in or a.web or a.es or a.commb or a.site or (a.aircraft and not a.modes) or (a.levels and a.modes)):
        ap.error("--replies works on samples and goes with --modes, --modes --aircraft, --levels, --beast and --avr only")
    if a.modes and not wire_in and not a.replies:
        ap.error("--modes needs --beast-in, --avr-in or --replies")
    if a.commb and not a.modes:
        ap.error("--commb needs --modes")
    if wire_in and a.levels and not a.aircraft:
        ap.error("--levels alone needs the samples")
    if a.es and not a.aircraft and (a.modes or a.web or a.levels):
        ap.error("--es without --aircraft prints lines of its own: not with --modes, --web or --levels")
    fmt = a.format or ("c16" if a.file.endswith(".c16") else "u8")
    st = A.ADSB_SAMPLE_I16 if fmt == "c16" else A.ADSB_SAMPLE_I8
    n_max = os.path.getsize(a.file) // (4 if fmt == "c16" else 2)
    if a.replies:
        d, frames, src, records = replies_run(a.device, st, read_capture(a.file, fmt),
                                                 levels="host" if a.levels else "device" if a.beast else None)
        with d:
            write_replies_wire(d, frames, a)
            if a.modes:
                recs = d.modes_of(frames)[0]
                sys.stdout.write(aircraft_table(d, frames, n_max, modes=recs) if a.aircraft else modes_lines(frames, recs))
            elif a.levels:
                sys.stdout.write(replies_level_lines(st, frames, records))
            else:
                sys.stdout.write(replies_lines(frames, src))
        if a.summary:
            n_replies = int(sum(1 for s in src if int(s) & A.ADSB_MERGE_FROM_B))
            print(f"{n_max} samples, {len(frames) - n_replies} packets, {n_replies} replies", file=sys.stderr)
        return
    with A.AdsbDemod(device=a.device, sample_type=st, max_samples=a.chunk + 240, max_out=a.chunk + 240,
                     host_staging=False) as d:
        if wire_in and a.modes:
            frames, recs, *regs = read_wire(d, a.file, wire_in, a.tick_bias, modes=True, commb=a.commb)
            if a.aircraft:
                n_samp = int(frames["offset"].max()) + A.WINDOW if len(frames) else 0
                sys.stdout.write(aircraft_table(d, frames, n_samp, site=a.site, modes=recs, commb=regs[0] if a.commb else None,
                                                es=d.es_of(frames)[0] if a.es else None))
            else:
                sys.stdout.write(modes_lines(frames, recs, regs[0] if a.commb else None))
            if a.summary:
                print(f"{os.path.getsize(a.file)} bytes, {len(frames)} frames", file=sys.stderr)
            return
        if wire_in:
            frames, parsed_levels = read_wire(d, a.file, wire_in, a.tick_bias)
            n_buf, n_samp = 0, (int(frames["offset"].max()) + A.WINDOW if len(frames) else 0)
            if a.aircraft:
                text = aircraft_table(d, frames, n_samp, st, parsed_levels if a.levels else None, site=a.site,
                                      es=d.es_of(frames)[0] if a.es else None)
            elif a.es:
                text = es_lines(frames, d.es_of(frames)[0])
            else:
                text = web_stream(d, frames, a.chunk) if a.web else stream_text(frames)
            write_wire(d, frames, a, fmt, parsed_levels)
            sys.stdout.write(text)
            if a.summary:
                print(f"{os.path.getsize(a.file)} bytes, {len(frames)} packets", file=sys.stderr)
            return
        frames, n_buf, n_samp, text = d.replay_file(a.file, L.ADSB_FILE_C16 if fmt == "c16" else L.ADSB_FILE_U8,
                                                    chunk_len=a.chunk, carry=a.carry, send_tail=a.tail,
                                                    max_frames=max(n_max // 200, 1 << 16))
        if a.aircraft and a.levels:
            text = aircraft_table(d, frames, n_samp, st, A.host_frame_levels(read_capture(a.file, fmt), frames),
                                  site=a.site, es=d.es_of(frames)[0] if a.es else None)
        elif a.aircraft:
            text = aircraft_table(d, frames, n_samp, site=a.site, es=d.es_of(frames)[0] if a.es else None)
        elif a.web:
            text = web_stream(d, frames, a.chunk)
        elif a.levels:
            text = level_lines(d, st, frames, read_capture(a.file, fmt))
        elif a.es:
            text = es_lines(frames, d.es_of(frames)[0])
        write_wire(d, frames, a, fmt)
    sys.stdout.write(text)
    if a.summary:
        print(f"{n_samp} samples, {n_buf} buffers of {a.chunk}, {len(frames)} packets", file=sys.stderr)


if __name__ == "__main__":
    main()
