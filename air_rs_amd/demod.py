"""Python face of the demodulator context (one per GPU, one per calling thread).

Mirrors the C ABI one to one; numpy arrays carry host buffers, integer device pointers (for
example ``torch.Tensor.data_ptr()``) carry HBM-resident ones.  Frames come back as a numpy
structured array with the adsb_frame layout.
"""
import collections
import ctypes as C
import math
import os

import numpy as np

from . import _lib as L

FRAME_DTYPE = np.dtype([("offset", "<u8"), ("bytes", "u1", (14,)), ("status", "u1"),
                        ("fixed_bit", "u1")])
assert FRAME_DTYPE.itemsize == C.sizeof(L.AdsbFrame) == 24

FIELDS_DTYPE = np.dtype([("icao", "<u4"), ("altitude", "<i4"), ("cpr_latitude", "<u4"), ("cpr_longitude", "<u4"),
                         ("downlink_format", "u1"), ("capability", "u1"), ("msg_type", "u1"), ("msg_kind", "u1"),
                         ("surveillance_status", "u1"), ("nic_supplement", "u1"), ("cpr_time", "u1"),
                         ("cpr_odd", "u1"), ("callsign", "S8")])
assert FIELDS_DTYPE.itemsize == C.sizeof(L.AdsbPacketFields) == 32

LEVEL_DTYPE = np.dtype([("signal_sum", "<u8"), ("noise_sum", "<u8"), ("peak", "<u4"), ("pulse_min", "<u4"),
                        ("quiet_max", "<u4"), ("weak_bits", "<u2"), ("flags", "<u2")])
assert LEVEL_DTYPE.itemsize == C.sizeof(L.AdsbFrameLevel) == 32
LEVEL_PULSE_SAMPLES, LEVEL_QUIET_SAMPLES = 116, 124  # of a frame's 240: what signal_sum and noise_sum add up
LEVEL_SHORT_PULSE_SAMPLES, LEVEL_SHORT_QUIET_SAMPLES = 60, 68  # of a 56-bit frame's 128 (ADSB_LEVEL_SHORT records)

SITE, FIX_DTYPE, FRAME_FIX_DTYPE = L.SITE, L.FIX_DTYPE, L.FRAME_FIX_DTYPE  # fixes_reserve / fixes / frame_fixes
AIRCRAFT_MLAT_DTYPE, FRAME_MLAT_DTYPE = L.AIRCRAFT_MLAT_DTYPE, L.FRAME_MLAT_DTYPE  # TrackTable.mlat / frame_mlat
AIRCRAFT_MODES_DTYPE = L.AIRCRAFT_MODES_DTYPE                                        # TrackTable.modes
AIRCRAFT_COMMB_DTYPE = L.AIRCRAFT_COMMB_DTYPE                                        # TrackTable.commb
WINDOW = 240  # 16 preamble + 112*2 samples (reference src/adsb.rs:98)


def synth_default(**overrides):
    cfg = L.AdsbSynthCfg()
    L.load().adsb_synth_default(C.byref(cfg))
    for k, v in overrides.items():
        if not hasattr(cfg, k):
            raise AttributeError(k)
        setattr(cfg, k, v)
    return cfg


def synth_fill_host(cfg, sample_type, channel, first_sample, n_samples):
    """Host copy of the synthetic stream: int8/int16 array of shape (n_samples, 2) = (I, Q)."""
    dt = np.int8 if sample_type == L.ADSB_SAMPLE_I8 else np.int16
    out = np.empty((n_samples, 2), dtype=dt)
    L.check(L.load().adsb_synth_fill_host(C.byref(cfg), sample_type, channel, first_sample,
                                          n_samples, out.ctypes.data), "adsb_synth_fill_host")
    return out


def _sample_type_of(iq):
    iq = np.asarray(iq)
    if iq.dtype == np.int8:
        return L.ADSB_SAMPLE_I8
    if iq.dtype == np.int16:
        return L.ADSB_SAMPLE_I16
    raise TypeError(f"IQ samples are int8 or int16, not {iq.dtype}")


def host_frame_levels(iq, frames, first_sample=0):
    """adsb_host_frame_levels, the CPU mirror of AdsbDemod.levels_of: one LEVEL_DTYPE record per frame of `frames`
    (FRAME_DTYPE) from the one-channel host buffer iq (int8 or int16, shape (n, 2)), whose sample 0 is stream sample
    first_sample.  A frame whose 240 samples are not all inside iq gets flags 0 and zeros."""
    st = _sample_type_of(iq)
    iq = np.ascontiguousarray(iq)
    n_samples = iq.size // 2
    frames = np.ascontiguousarray(frames, dtype=FRAME_DTYPE)
    out = np.zeros(max(len(frames), 1), dtype=LEVEL_DTYPE)
    keep = iq if iq.size else np.zeros(2, dtype=iq.dtype)      # a non-NULL pointer for an empty buffer
    L.check(L.load().adsb_host_frame_levels(st, keep.ctypes.data, n_samples, int(first_sample),
                                            frames.ctypes.data if len(frames) else None, len(frames),
                                            out.ctypes.data_as(C.POINTER(L.AdsbFrameLevel))), "adsb_host_frame_levels")
    return out[:len(frames)].copy()


def _channel_counts(counts, n):
    """counts as a flat uint64 array; None: one channel of n frames.  Nothing is checked here: the library refuses
    counts that do not add up to the list's length."""
    return np.array([n], dtype=np.uint64) if counts is None else np.ascontiguousarray(counts, dtype=np.uint64).reshape(-1)


def host_frame_levels_modes(iq, frames, counts=None, n_samples=None, channel_stride=None, first_sample=0):
    """adsb_host_frame_levels_modes, the CPU mirror of AdsbDemod.levels_modes_of: one LEVEL_DTYPE record per frame of
    `frames` (FRAME_DTYPE, in channel order, counts[c] of channel c; None: one channel), a 56-bit frame's over its 128
    samples with ADSB_LEVEL_SHORT, a 112-bit frame's as host_frame_levels.  iq: int8 or int16 host samples, channel c
    starting channel_stride samples after channel c-1 (default: n_samples).  n_samples may be left out for one channel
    only (all of iq); with more channels it must be given, and iq must hold the last channel whole."""
    st = _sample_type_of(iq)
    iq = np.ascontiguousarray(iq)
    frames = np.ascontiguousarray(frames, dtype=FRAME_DTYPE)
    counts = _channel_counts(counts, len(frames))
    if n_samples is None:
        if len(counts) != 1:
            raise ValueError("n_samples is needed with more than one channel")
        n_samples = iq.size // 2
    stride = n_samples if channel_stride is None else channel_stride
    if len(counts) and (len(counts) - 1) * stride + n_samples > iq.size // 2:
        raise ValueError(f"iq holds {iq.size // 2} samples, {len(counts)} channels of {n_samples} at stride {stride} need more")
    out = np.zeros(max(len(frames), 1), dtype=LEVEL_DTYPE)
    keep = iq if iq.size else np.zeros(2, dtype=iq.dtype)
    L.check(L.load().adsb_host_frame_levels_modes(st, keep.ctypes.data, len(counts), int(n_samples), int(stride),
                                                  int(first_sample), frames.ctypes.data if len(frames) else None,
                                                  counts.ctypes.data if len(counts) else None, len(frames),
                                                  out.ctypes.data), "adsb_host_frame_levels_modes")
    return out[:len(frames)].copy()


def _sites(sites, n):
    """n sites as a SITE array: a SITE array, or (latitude, longitude[, max_range_nm = 180]) tuples."""
    if isinstance(sites, np.ndarray) and sites.dtype == SITE:
        out = np.ascontiguousarray(sites).reshape(-1)
    else:
        out = np.zeros(len(sites), dtype=SITE)
        for k, site in enumerate(sites):
            site = tuple(site)
            out[k] = (site[0], site[1], site[2] if len(site) > 2 else 180.0)
    if len(out) != n:
        raise ValueError(f"sites: {len(out)} for {n} receivers")
    return out


def host_fix_of(site, frame_bytes, time=0.0):
    """adsb_host_fix_of, the CPU mirror of a fixes reserve's per-frame decode: (FIX_DTYPE record of an aircraft whose
    only frame is this one, heard at `time` from `site`; the frame's FRAME_FIX_DTYPE flags).  site: (latitude,
    longitude[, max_range_nm = 180]) or a SITE record.  Needs no device."""
    s = _sites(site.reshape(-1) if isinstance(site, np.ndarray) else [site], 1)
    b = (C.c_uint8 * 14)(*bytes(frame_bytes))
    out = np.zeros(1, dtype=FIX_DTYPE)
    flags = C.c_uint32()
    L.check(L.load().adsb_host_fix_of(s.ctypes.data_as(C.POINTER(L.AdsbSite)), C.byref(b), float(time),
                                      out.ctypes.data_as(C.POINTER(L.AdsbFix)), C.byref(flags)), "adsb_host_fix_of")
    return out[0], flags.value


def host_track_mlat_of(max_disagreement_m, frame_bytes, fix, time=0.0):
    """adsb_host_track_mlat_of, the CPU mirror of an mlat reserve's per-frame step: (AIRCRAFT_MLAT_DTYPE record of an
    aircraft whose only counted frame is this one with the MLAT_FIX_DTYPE record `fix`, heard at `time`; the frame's
    FRAME_MLAT_DTYPE flags; its disagreement_m as np.float32).  Needs no device."""
    b = (C.c_uint8 * 14)(*bytes(frame_bytes))
    f = np.zeros(1, dtype=L.MLAT_FIX_DTYPE)
    f[0] = fix
    out = np.zeros(1, dtype=AIRCRAFT_MLAT_DTYPE)
    flags, dis = C.c_uint32(), C.c_float()
    L.check(L.load().adsb_host_track_mlat_of(float(max_disagreement_m), C.byref(b),
                                             f.ctypes.data_as(C.POINTER(L.AdsbMlatFix)), float(time),
                                             out.ctypes.data_as(C.POINTER(L.AdsbAircraftMlat)), C.byref(flags),
                                             C.byref(dis)), "adsb_host_track_mlat_of")
    return out[0], flags.value, np.float32(dis.value)


AIRCRAFT_FILTER_DTYPE, FRAME_FILTER_DTYPE = L.AIRCRAFT_FILTER_DTYPE, L.FRAME_FILTER_DTYPE  # TrackTable.filter / frame_filter
FILTER_OPERAND_DTYPE = L.FILTER_OPERAND_DTYPE
FILTER_CFG_FIELDS = tuple(name for name, _ in L.AdsbTrackFilterCfg._fields_ if name != "reserved")


def _filter_cfg(**cfg):
    """An adsb_track_filter_cfg of keyword arguments (FILTER_CFG_FIELDS); what is not given is 0, the default."""
    unknown = set(cfg) - set(FILTER_CFG_FIELDS)
    if unknown:
        raise TypeError(f"filter cfg: unknown field(s) {sorted(unknown)}")
    c = L.AdsbTrackFilterCfg()
    for name, value in cfg.items():
        setattr(c, name, int(value) if name in ("max_outliers", "min_run") else float(value))
    return c


def filter_empty(n=1):
    """n EMPTY AIRCRAFT_FILTER_DTYPE records: all zeros with time NaN."""
    out = np.zeros(n, dtype=AIRCRAFT_FILTER_DTYPE)
    out["time"] = np.nan
    return out


def host_track_filter_operand(fix, time, counted=True, **cfg):
    """adsb_host_track_filter_operand, the CPU mirror of a filter reserve's per-frame kernel: the FILTER_OPERAND_DTYPE
    record of a frame with the MLAT_FIX_DTYPE record `fix` at frame time `time`.  Needs no device."""
    f = np.zeros(1, dtype=L.MLAT_FIX_DTYPE)
    f[0] = fix
    out = np.zeros(1, dtype=FILTER_OPERAND_DTYPE)
    c = _filter_cfg(**cfg)
    L.check(L.load().adsb_host_track_filter_operand(C.byref(c), f.ctypes.data_as(C.POINTER(L.AdsbMlatFix)), float(time),
                                                    1 if counted else 0,
                                                    out.ctypes.data_as(C.POINTER(L.AdsbFilterOperand))),
            "adsb_host_track_filter_operand")
    return out[0]


def host_track_filter_step(record, operand, **cfg):
    """adsb_host_track_filter_step, the CPU mirror of one step of a filter reserve's walk: (the AIRCRAFT_FILTER_DTYPE
    record after a frame with the FILTER_OPERAND_DTYPE record `operand`, that frame's FRAME_FILTER_DTYPE record).
    record: the aircraft's so far (filter_empty()[0] for none).  Needs no device."""
    r = np.zeros(1, dtype=AIRCRAFT_FILTER_DTYPE)
    r[0] = record
    o = np.zeros(1, dtype=FILTER_OPERAND_DTYPE)
    o[0] = operand
    f = np.zeros(1, dtype=FRAME_FILTER_DTYPE)
    c = _filter_cfg(**cfg)
    L.check(L.load().adsb_host_track_filter_step(C.byref(c), r.ctypes.data_as(C.POINTER(L.AdsbAircraftFilter)),
                                                 o.ctypes.data_as(C.POINTER(L.AdsbFilterOperand)),
                                                 f.ctypes.data_as(C.POINTER(L.AdsbFrameFilter))),
            "adsb_host_track_filter_step")
    return r[0], f[0]


FILTER_PHYSICAL_DTYPE = np.dtype([("ground_speed_kt", "<f8"), ("track_deg", "<f8"), ("vertical_rate_fpm", "<f8"),
                                  ("position_sigma_m", "<f8"), ("speed_sigma_kt", "<f8")])


def filter_physical(recs):
    """AIRCRAFT_FILTER_DTYPE records in the units a display shows -> FILTER_PHYSICAL_DTYPE: ground speed in knots, track
    in degrees clockwise from north in [0, 360), vertical rate in ft/min, and the 1-sigma of the horizontal position
    (metres) and of the ground speed (knots) from the covariance's diagonals.  NaN where ADSB_TRACK_FILTER_VELOCITY is
    unset (position_sigma_m: where RUNNING is)."""
    recs = np.atleast_1d(np.asarray(recs, dtype=AIRCRAFT_FILTER_DTYPE))
    out = np.full(len(recs), np.nan, dtype=FILTER_PHYSICAL_DTYPE)
    running = (recs["flags"] & L.ADSB_TRACK_FILTER_RUNNING) != 0
    vel = (recs["flags"] & L.ADSB_TRACK_FILTER_VELOCITY) != 0
    kt = 3600.0 / 1852.0
    vn, ve = recs["v_north"], recs["v_east"]
    out["ground_speed_kt"][vel] = (np.hypot(vn, ve) * kt)[vel]
    out["track_deg"][vel] = (np.degrees(np.arctan2(ve, vn)) % 360.0)[vel]
    out["vertical_rate_fpm"][vel] = (recs["v_up"] * (60.0 / 0.3048))[vel]
    out["position_sigma_m"][running] = np.sqrt(recs["p_north"][:, 0] + recs["p_east"][:, 0])[running]
    out["speed_sigma_kt"][vel] = (np.sqrt((recs["p_north"][:, 2] + recs["p_east"][:, 2]) / 2.0) * kt)[vel]
    return out


def host_track_modes_of(rec, time=0.0):
    """adsb_host_track_modes_of, the CPU mirror of a modes reserve's per-frame step: (AIRCRAFT_MODES_DTYPE record of an
    aircraft whose only counted frame is the one with the MODES_DTYPE record `rec`, heard at `time`; whether the frame
    is accepted).  Needs no device."""
    r = np.zeros(1, dtype=MODES_DTYPE)
    r[0] = rec
    out = np.zeros(1, dtype=AIRCRAFT_MODES_DTYPE)
    ok = C.c_uint32()
    L.check(L.load().adsb_host_track_modes_of(r.ctypes.data, float(time), out.ctypes.data_as(C.POINTER(L.AdsbAircraftModes)),
                                              C.byref(ok)), "adsb_host_track_modes_of")
    return out[0].copy(), bool(ok.value)


def host_track_modes_merge(into, later):
    """adsb_host_track_modes_merge, the combine of a modes reserve: the AIRCRAFT_MODES_DTYPE record `into` followed by
    `later`, a record of the frames that come after into's.  Needs no device."""
    a, b = np.zeros(1, dtype=AIRCRAFT_MODES_DTYPE), np.zeros(1, dtype=AIRCRAFT_MODES_DTYPE)
    a[0], b[0] = into, later
    P = C.POINTER(L.AdsbAircraftModes)
    L.check(L.load().adsb_host_track_modes_merge(a.ctypes.data_as(P), b.ctypes.data_as(P)), "adsb_host_track_modes_merge")
    return a[0].copy()


WIRE_FORMATS = {"beast": L.ADSB_WIRE_BEAST, "avr": L.ADSB_WIRE_AVR, "avr_mlat": L.ADSB_WIRE_AVR_MLAT}


def _wire_cfg(format, signal, tick_bias, short=False):
    fmt = WIRE_FORMATS[format] if isinstance(format, str) else int(format)
    return L.AdsbWireCfg(fmt | (L.ADSB_WIRE_SHORT if short else 0), 1 if signal else 0, int(tick_bias))


def _host_list(arr, dtype, n=None):
    """(array kept alive, pointer or None, count) of a host record list."""
    arr = np.ascontiguousarray(arr, dtype=dtype)
    if n is not None and len(arr) != n:
        raise ValueError(f"{len(arr)} level records for {n} frames")
    return arr, (arr.ctypes.data if len(arr) else None), len(arr)


def host_wire_encode(frames, levels=None, format="beast", sample_type=L.ADSB_SAMPLE_I8, tick_bias=0, cap=None,
                     short=False):
    """adsb_host_wire_encode, the CPU mirror of AdsbDemod.wire_of: (stream as bytes, ends as a uint32 array) of the
    FRAME_DTYPE list `frames` with their LEVEL_DTYPE records `levels` (None: signal byte 0; sample_type gives its full
    scale).  cap (default: enough): room in the output; with less than the stream needs, `bytes` holds the longest
    prefix of whole frames and `ends` still has every frame's end.  short: ADSB_WIRE_SHORT, 56-bit frames leave as
    short frames (Beast '2', 14 hex digits).  Needs no device."""
    frames, fptr, n = _host_list(frames, FRAME_DTYPE)
    lptr = None
    if levels is not None:
        levels, lptr, _ = _host_list(levels, LEVEL_DTYPE, n)
    cfg = _wire_cfg(format, levels is not None, tick_bias, short)
    room = L.ADSB_WIRE_MAX_BYTES * n if cap is None else int(cap)
    out = np.zeros(max(room, 1), dtype=np.uint8)
    ends = np.zeros(max(n, 1), dtype=np.uint32)
    total = C.c_size_t()
    L.check(L.load().adsb_host_wire_encode(C.byref(cfg), int(sample_type), fptr, lptr, n, out.ctypes.data, room,
                                           C.byref(total), ends.ctypes.data), "adsb_host_wire_encode")
    return _wire_result(out, room, ends[:n].copy(), total.value)


def _wire_result(out, room, ends, total):
    """The bytes the call wrote: the stream, or its longest prefix of whole frames within `room`."""
    if total > room:
        fit = ends[ends <= room]
        total = int(fit[-1]) if len(fit) else 0
    return out[:total].tobytes(), ends


WIRE_RX_DTYPE = np.dtype([("ticks", "<u8"), ("pos", "<u4"), ("signal", "u1"), ("kind", "u1"), ("receiver", "<u2")])
assert WIRE_RX_DTYPE.itemsize == C.sizeof(L.AdsbWireRx) == 16
WIRE_IN_HEADER_DTYPE = np.dtype([(k, "<u8") for k in ("n_frames", "total_found", "n_marks", "n_cut", "n_unknown",
                                                       "n_other", "n_rejected", "flags")])
assert WIRE_IN_HEADER_DTYPE.itemsize == C.sizeof(L.AdsbWireInHeader) == 64
WIRE_IN_FILTERS = {"crc": L.ADSB_WIRE_IN_CRC, "df17": L.ADSB_WIRE_IN_DF17, "short": L.ADSB_WIRE_IN_SHORT}
WIRE_IN_SHORT = L.ADSB_WIRE_IN_SHORT     # filter bit: also emit the 56-bit frames (Mode S replies; see modes_of)
WireIn = collections.namedtuple("WireIn", "frames rx levels counts consumed header")
WireIn.__doc__ = """One parse of wire input: FRAME_DTYPE frames, WIRE_RX_DTYPE rx, LEVEL_DTYPE levels (None without
levels=True), uint64 counts and consumed per stream, and the WIRE_IN_HEADER_DTYPE record."""


def _wire_in_cfg(format, filter, tick_bias, max_frames, sample_type, levels):
    fmt = WIRE_FORMATS[format] if isinstance(format, str) else int(format)
    if isinstance(filter, str):
        filter = [filter]
    bits = int(filter) if isinstance(filter, int) else sum(WIRE_IN_FILTERS[f] for f in (filter or ()))
    return L.AdsbWireInCfg(fmt, bits, int(tick_bias), int(max_frames), int(sample_type), 1 if levels else 0)


def _wire_in_input(data, stream_ends):
    """(array kept alive or None, pointer or None, n_bytes, uint64 ends) of bytes-like / uint8 array / (device pointer,
    length) input; stream_ends None: one stream."""
    if isinstance(data, tuple):
        keep, ptr, n = None, int(data[0]), int(data[1])
    else:
        keep = np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else \
            np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
        ptr, n = (keep.ctypes.data if len(keep) else None), len(keep)
    ends = np.ascontiguousarray([n] if stream_ends is None else stream_ends, dtype=np.uint64).reshape(-1)
    return keep, (ptr if n else None), n, ends


def _wire_in_room(n_bytes, max_frames, levels, filter_bits=0):
    most = n_bytes // (16 if filter_bits & L.ADSB_WIRE_IN_SHORT else 23)      # the shortest emitted frame
    room = most if not max_frames else min(int(max_frames), most)
    return (room, np.zeros(max(room, 1), dtype=FRAME_DTYPE), np.zeros(max(room, 1), dtype=WIRE_RX_DTYPE),
            np.zeros(max(room, 1), dtype=LEVEL_DTYPE) if levels else None)


def _wire_in_result(fr, rx, lv, n, counts, consumed, hdr):
    header = np.frombuffer(bytes(hdr), dtype=WIRE_IN_HEADER_DTYPE)[0]
    return WireIn(fr[:n].copy(), rx[:n].copy(), None if lv is None else lv[:n].copy(), counts, consumed, header)


def host_wire_parse(data, stream_ends=None, format="beast", filter=0, tick_bias=0, max_frames=0,
                    sample_type=L.ADSB_SAMPLE_I8, levels=False):
    """adsb_host_wire_parse, the CPU mirror of AdsbDemod.wire_in_of: one or many streams of Beast binary ("beast") or AVR
    text ("avr", "avr_mlat": both read '*' and '@' lines) laid end to end in `data` (bytes-like or a uint8 array), with
    their ascending exclusive ends (None: one stream), back into a WireIn.  filter: 0, "crc", "df17", a list of those or
    the ADSB_WIRE_IN_* bits; levels: level records from the signal bytes, on sample_type's full scale.  Needs no
    device."""
    keep, ptr, n, ends = _wire_in_input(data, stream_ends)
    cfg = _wire_in_cfg(format, filter, tick_bias, max_frames, sample_type, levels)
    room, fr, rx, lv = _wire_in_room(n, max_frames, levels, cfg.filter)
    counts, consumed = np.zeros(len(ends), dtype=np.uint64), np.zeros(len(ends), dtype=np.uint64)
    got, hdr = C.c_size_t(), L.AdsbWireInHeader()
    L.check(L.load().adsb_host_wire_parse(C.byref(cfg), ptr, n, ends.ctypes.data if len(ends) else None, len(ends),
                                          fr.ctypes.data, rx.ctypes.data, None if lv is None else lv.ctypes.data, room,
                                          C.byref(got), counts.ctypes.data if len(ends) else None,
                                          consumed.ctypes.data if len(ends) else None, C.byref(hdr)),
            "adsb_host_wire_parse")
    return _wire_in_result(fr, rx, lv, got.value, counts, consumed, hdr)


MODES_DTYPE = np.dtype([("address", "<u4"), ("df", "u1"), ("kind", "u1"), ("flags", "<u2"), ("altitude_ft", "<i4"),
                        ("squawk", "<u2"), ("fs", "u1"), ("dr", "u1"), ("um", "u1"), ("iid", "u1"), ("ca", "u1"), ("ri", "u1"),
                        ("callsign", "S8"), ("reserved", "u1", (4,))])
assert MODES_DTYPE.itemsize == C.sizeof(L.AdsbModesRec) == 32
MODES_HEADER_DTYPE = np.dtype([(k, "<u8") for k in ("n", "n_self", "n_known", "n_unknown", "n_parity", "n_unsupported",
                                                     "n_known_out", "n_squitters")])
assert MODES_HEADER_DTYPE.itemsize == C.sizeof(L.AdsbModesHeader) == 64
MODES_KINDS = ("SELF", "KNOWN", "UNKNOWN", "PARITY", "UNSUPPORTED")


def _known_list(known):
    """(array kept alive or None, pointer or None, count) of a known-address argument: None, an ascending unique uint32
    array, a (device pointer, count) pair, or a TrackTable, whose fetched ICAOs are used."""
    if known is None:
        return None, None, 0
    if isinstance(known, tuple):
        return None, (int(known[0]) if int(known[1]) else None), int(known[1])
    if hasattr(known, "aircraft") and not hasattr(known, "dtype"):
        known = np.unique(np.asarray(known.aircraft()[0]["icao"], dtype=np.uint32))     # (the table lists ascending ICAOs)
    arr = np.ascontiguousarray(known, dtype=np.uint32).reshape(-1)
    return arr, (arr.ctypes.data if len(arr) else None), len(arr)


def host_modes(frames, counts=None, known=None):
    """adsb_host_modes, the CPU mirror of AdsbDemod.modes_of: (MODES_DTYPE records, uint32 known_out, FRAME_DTYPE
    squitters, uint64 squitter_counts or None, the MODES_HEADER_DTYPE record) of the FRAME_DTYPE list `frames`; counts[r]
    frames per receiver (None: no squitter_counts); known: None or an ascending unique uint32 array of addresses.  Needs
    no device."""
    frames, fptr, n = _host_list(frames, FRAME_DTYPE)
    karr, kptr, nk = _known_list(known)
    cnt = None if counts is None else np.ascontiguousarray(counts, dtype=np.uint64).reshape(-1)
    recs, kout = np.zeros(max(n, 1), dtype=MODES_DTYPE), np.zeros(max(n + nk, 1), dtype=np.uint32)
    sq = np.zeros(max(n, 1), dtype=FRAME_DTYPE)
    sqc = None if cnt is None else np.zeros(max(len(cnt), 1), dtype=np.uint64)
    hdr = L.AdsbModesHeader()
    L.check(L.load().adsb_host_modes(fptr, n, None if cnt is None else cnt.ctypes.data, 0 if cnt is None else len(cnt),
                                     kptr, nk, recs.ctypes.data, kout.ctypes.data, sq.ctypes.data,
                                     None if sqc is None else sqc.ctypes.data, C.byref(hdr)), "adsb_host_modes")
    header = np.frombuffer(bytes(hdr), dtype=MODES_HEADER_DTYPE)[0]
    return (recs[:n].copy(), kout[:int(header["n_known_out"])].copy(), sq[:int(header["n_squitters"])].copy(),
            None if sqc is None else sqc[:len(cnt)].copy(), header)


COMMB_DTYPE = np.dtype([("state", "u1"), ("bds", "u1"), ("candidates", "u1"), ("n_candidates", "u1"), ("status", "<u2"),
                        ("reserved", "<u2"), ("value", "<i4", (5,)), ("word", "<u4")])
assert COMMB_DTYPE.itemsize == C.sizeof(L.AdsbCommbRec) == 32
COMMB_HEADER_DTYPE = np.dtype([(k, "<u8") for k in ("n", "n_commb", "n_empty", "n_none", "n_one", "n_ambiguous")]
                              + [("n_bds", "<u8", (7,)), ("reserved", "<u8", (3,))])
assert COMMB_HEADER_DTYPE.itemsize == C.sizeof(L.AdsbCommbHeader) == 128
COMMB_STATES = ("NOT_COMMB", "EMPTY", "NONE", "ONE", "AMBIGUOUS")
COMMB_REGISTERS = (0x10, 0x17, 0x20, 0x30, 0x40, 0x50, 0x60)     # in the order of the candidate bits and of n_bds
# commb_physical: key -> (register, index into value[], what one unit of the value is in the key's unit)
_COMMB_PHYSICAL = {
    "mcp_altitude_ft": (0x40, 0, 1.0), "fms_altitude_ft": (0x40, 1, 1.0), "baro_setting_mb": (0x40, 2, 0.1),
    "roll_deg": (0x50, 0, 45.0 / 256.0), "true_track_deg": (0x50, 1, 90.0 / 512.0),
    "ground_speed_kt": (0x50, 2, 1.0), "track_rate_deg_s": (0x50, 3, 8.0 / 256.0),
    "true_airspeed_kt": (0x50, 4, 1.0),
    "magnetic_heading_deg": (0x60, 0, 90.0 / 512.0), "ias_kt": (0x60, 1, 1.0), "mach": (0x60, 2, 0.004),
    "baro_rate_ft_min": (0x60, 3, 1.0), "inertial_rate_ft_min": (0x60, 4, 1.0),
}


def host_commb(frames):
    """adsb_host_commb, the CPU mirror of AdsbDemod.commb_of: (COMMB_DTYPE records, the COMMB_HEADER_DTYPE record) of
    the FRAME_DTYPE list `frames`.  Needs no device."""
    frames, fptr, n = _host_list(frames, FRAME_DTYPE)
    recs, hdr = np.zeros(max(n, 1), dtype=COMMB_DTYPE), L.AdsbCommbHeader()
    L.check(L.load().adsb_host_commb(fptr, n, recs.ctypes.data, C.byref(hdr)), "adsb_host_commb")
    return recs[:n].copy(), np.frombuffer(bytes(hdr), dtype=COMMB_HEADER_DTYPE)[0]


def host_commb_as(frame_bytes, bds):
    """adsb_host_commb_as: the COMMB_DTYPE record of one frame's 14 bytes with MB decoded as register `bds` (0x10 ...
    0x60), whatever the inference says; AdsbError(ADSB_E_ARG) if `bds` is not among the frame's candidates.  What a
    consumer that knows more settles an AMBIGUOUS record with.  Needs no device."""
    b = np.zeros(14, dtype=np.uint8)
    raw = np.frombuffer(bytes(frame_bytes), dtype=np.uint8)[:14]
    b[:len(raw)] = raw
    rec = np.zeros(1, dtype=COMMB_DTYPE)
    L.check(L.load().adsb_host_commb_as(b.ctypes.data, int(bds), rec.ctypes.data), "adsb_host_commb_as")
    return rec[0]


def commb_physical(recs):
    """The values of COMMB_DTYPE records in physical units: a dict of float64 arrays, one entry per record, NaN where
    the status bit is off, the state is not ONE or the register is another.  BDS 4,0: mcp_altitude_ft, fms_altitude_ft,
    baro_setting_mb.  BDS 5,0: roll_deg, true_track_deg, ground_speed_kt, track_rate_deg_s, true_airspeed_kt.  BDS
    6,0: magnetic_heading_deg, ias_kt, mach, baro_rate_ft_min, inertial_rate_ft_min."""
    recs = np.atleast_1d(np.asarray(recs, dtype=COMMB_DTYPE))
    one = recs["state"] == L.ADSB_COMMB_ONE
    out = {}
    for key, (bds, k, factor) in _COMMB_PHYSICAL.items():
        held = one & (recs["bds"] == bds) & ((recs["status"] >> k) & 1 == 1)
        out[key] = np.where(held, recs["value"][:, k] * factor, np.nan)
    return out


ES_DTYPE = np.dtype([("state", "u1"), ("type_code", "u1"), ("subtype", "u1"), ("version", "u1"), ("present", "<u4")]
                    + [(k, "u1") for k in ("nic_a", "nic_b", "nic_c", "nac_p", "nac_v", "sil", "sil_supplement", "gva", "sda",
                                           "nic_baro", "category", "emergency", "length_width", "reserved")]
                    + [("flags", "<u2"), ("value", "<u4"), ("half", "<u2", (2,))])
assert ES_DTYPE.itemsize == C.sizeof(L.AdsbEsRec) == 32
ES_HEADER_DTYPE = np.dtype([("n", "<u8"), ("n_state", "<u8", (10,)), ("n_version", "<u8", (4,)), ("reserved", "<u8")])
assert ES_HEADER_DTYPE.itemsize == C.sizeof(L.AdsbEsHeader) == 128
ES_STATES = ("NOT_ES", "FOREIGN", "CATEGORY", "POSITION", "VELOCITY", "EMERGENCY", "ACAS_RA", "TARGET_STATE", "OPERATIONAL",
             "RESERVED")
# es_physical: key -> (present bit, field, index into it or None, what one unit of the value is in the key's unit)
_ES_PHYSICAL = {
    "rc_m": (L.ADSB_ES_HAS_RC, "value", None, 0.1),
    "selected_altitude_ft": (L.ADSB_ES_HAS_SELECTED_ALT, "value", None, 1.0),
    "baro_setting_mb": (L.ADSB_ES_HAS_BARO, "half", 0, 0.1),
    "selected_heading_deg": (L.ADSB_ES_HAS_HEADING, "half", 1, 180.0 / 256.0),
}


def host_es(frames):
    """adsb_host_es, the CPU mirror of AdsbDemod.es_of: (ES_DTYPE records, the ES_HEADER_DTYPE record) of the
    FRAME_DTYPE list `frames`.  Needs no device."""
    frames, fptr, n = _host_list(frames, FRAME_DTYPE)
    recs, hdr = np.zeros(max(n, 1), dtype=ES_DTYPE), L.AdsbEsHeader()
    L.check(L.load().adsb_host_es(fptr, n, recs.ctypes.data, C.byref(hdr)), "adsb_host_es")
    return recs[:n].copy(), np.frombuffer(bytes(hdr), dtype=ES_HEADER_DTYPE)[0]


def host_es_integrity(tc, version, supp=0):
    """adsb_host_es_integrity: (NIC, Rc in decimetres, 0 for unknown) of a position message with type code `tc` from an
    aircraft of ADS-B `version` (ADSB_ES_VERSION_UNKNOWN reads as 0) with the NIC supplements `supp` (bit 0 = A, bit 1 =
    B, bit 2 = C).  Needs no device."""
    nic, rc = C.c_uint32(), C.c_uint32()
    L.check(L.load().adsb_host_es_integrity(int(tc), int(version), int(supp), C.byref(nic), C.byref(rc)), "adsb_host_es_integrity")
    return nic.value, rc.value


def es_physical(recs):
    """The values of ES_DTYPE records in physical units: a dict of float64 arrays, one entry per record, NaN where the
    record does not hold the value (its present bit is off).  POSITION: rc_m, the containment radius the type code alone
    gives, in metres.  TARGET_STATE: selected_altitude_ft, baro_setting_mb, selected_heading_deg."""
    recs = np.atleast_1d(np.asarray(recs, dtype=ES_DTYPE))
    out = {}
    for key, (bit, field, k, factor) in _ES_PHYSICAL.items():
        raw = recs[field] if k is None else recs[field][:, k]
        out[key] = np.where(recs["present"] & bit != 0, raw * factor, np.nan)
    return out


REPLIES_HEADER_DTYPE = np.dtype([(k, "<u8") for k in ("n_out", "total_found", "n_preamble", "n_all_call", "n_df18",
                                                      "n_address_parity", "n_not_known", "n_parity", "flags", "reserved")])
assert REPLIES_HEADER_DTYPE.itemsize == C.sizeof(L.AdsbRepliesHeader) == 80
REPLIES_AP = {"all": 0, "known": L.ADSB_REPLIES_AP_KNOWN}     # replies_of's `ap`: the address/parity formats kept


def _replies_cfg(ap, max_frames, first_sample):
    if ap not in REPLIES_AP:
        raise ValueError(f"ap must be one of {sorted(REPLIES_AP)}, not {ap!r}")
    return L.AdsbRepliesCfg(REPLIES_AP[ap], 0, int(max_frames), int(first_sample), 0)


def host_replies(iq, n_channels=1, n_samples=None, channel_stride=None, known=None, ap="all", max_frames=0, first_sample=0):
    """adsb_host_replies, the CPU mirror of AdsbDemod.replies_of: (FRAME_DTYPE frames, uint64 counts per channel, the
    REPLIES_HEADER_DTYPE record) of the host samples `iq` (int8 or int16, [samples, 2] or flat I,Q pairs; n_channels
    buffers of n_samples samples, channel_stride samples apart).  known: None or an ascending unique uint32 array;
    ap: "all" or "known".  Needs no device."""
    iq = np.ascontiguousarray(iq)
    if iq.dtype not in (np.int8, np.int16):
        raise ValueError("iq must be int8 or int16")
    st = L.ADSB_SAMPLE_I8 if iq.dtype == np.int8 else L.ADSB_SAMPLE_I16
    total = iq.size // 2
    n_samples = total // int(n_channels) if n_samples is None else int(n_samples)
    stride = n_samples if channel_stride is None else int(channel_stride)
    if (int(n_channels) - 1) * stride + n_samples > total:
        raise ValueError("iq is shorter than the channels say")
    karr, kptr, nk = _known_list(known)
    cfg, hdr, fn = _replies_cfg(ap, max_frames, first_sample), L.AdsbRepliesHeader(), L.load().adsb_host_replies
    counts = np.zeros(max(int(n_channels), 1), dtype=np.uint64)
    args = (st, C.byref(cfg), iq.ctypes.data, int(n_channels), n_samples, stride, kptr, nk)
    L.check(fn(*args, None, 0, None, None, C.byref(hdr)), "adsb_host_replies")          # the size first
    n = int(hdr.n_out)
    out = np.zeros(max(n, 1), dtype=FRAME_DTYPE)
    L.check(fn(*args, out.ctypes.data, n, None, counts.ctypes.data, C.byref(hdr)), "adsb_host_replies")
    return out[:n].copy(), counts[:int(n_channels)].copy(), np.frombuffer(bytes(hdr), dtype=REPLIES_HEADER_DTYPE)[0]


def host_merge_lists(a, counts_a, b, counts_b):
    """adsb_host_merge_lists, the CPU mirror of AdsbDemod.merge_lists: two FRAME_DTYPE lists in fetch's layout (frames
    per channel in counts_a / counts_b, each channel in ascending offset) as one -> (frames, src, counts): on equal
    offsets a's frame first; src[k] = the index of frames[k] in its own list, ADSB_MERGE_FROM_B set for b's.  Needs no
    device."""
    a, aptr, na = _host_list(a, FRAME_DTYPE)
    b, bptr, nb = _host_list(b, FRAME_DTYPE)
    ca, cb = (np.ascontiguousarray(x, dtype=np.uint64).reshape(-1) for x in (counts_a, counts_b))
    if len(ca) != len(cb) or int(ca.sum()) != na or int(cb.sum()) != nb:
        raise ValueError("counts do not describe the lists")
    out, src = np.zeros(max(na + nb, 1), dtype=FRAME_DTYPE), np.zeros(max(na + nb, 1), dtype=np.uint32)
    counts = np.zeros(max(len(ca), 1), dtype=np.uint64)
    L.check(L.load().adsb_host_merge_lists(aptr, ca.ctypes.data, bptr, cb.ctypes.data, len(ca), out.ctypes.data,
                                           src.ctypes.data, counts.ctypes.data), "adsb_host_merge_lists")
    return out[:na + nb].copy(), src[:na + nb].copy(), counts[:len(ca)].copy()


FRAME_INTEGRITY_DTYPE = np.dtype([("rc_dm", "<u4"), ("nic", "u1"), ("version", "u1"), ("supp", "u1"), ("flags", "u1")])
AIRCRAFT_ES_DTYPE = np.dtype([(k, ES_DTYPE) for k in ("operational_airborne", "operational_surface", "target_state",
                                                      "emergency", "acas_ra")]
                             + [("time", "<f8", (5,))]
                             + [(k, "<f8") for k in ("version_time", "nic_a_time", "nic_c_time", "position_time")]
                             + [("rc_dm", "<u4")]
                             + [(k, "u1") for k in ("nic", "position_tc", "nic_b", "position_supp", "version", "nic_a",
                                                    "nic_c", "category")]
                             + [("n_es", "<u4"), ("n_position", "<u4")]
                             + [(k, "u1") for k in ("nac_v", "velocity_flags", "has", "reserved")])
assert FRAME_INTEGRITY_DTYPE.itemsize == C.sizeof(L.AdsbFrameIntegrity) == 8
assert AIRCRAFT_ES_DTYPE.itemsize == C.sizeof(L.AdsbAircraftEs) == 256
AIRCRAFT_ES_BLOCKS = ("operational_airborne", "operational_surface", "target_state", "emergency", "acas_ra")


def host_es_resolve(rec, time=0.0, held=None, max_age_s=60.0):
    """adsb_host_es_resolve, the CPU mirror of an es reserve's resolution: the FRAME_INTEGRITY_DTYPE record of a frame
    with the ES_DTYPE record `rec` heard at `time`, of an aircraft whose AIRCRAFT_ES_DTYPE record before the frame is
    `held` (None: the empty record).  Needs no device."""
    r = np.array([rec], dtype=ES_DTYPE)
    h = None if held is None else np.array([held], dtype=AIRCRAFT_ES_DTYPE)
    cfg = L.AdsbEsTrackCfg(float(max_age_s))
    out = np.zeros(1, dtype=FRAME_INTEGRITY_DTYPE)
    L.check(L.load().adsb_host_es_resolve(r.ctypes.data, float(time), None if h is None else h.ctypes.data, C.byref(cfg),
                                          out.ctypes.data), "adsb_host_es_resolve")
    return out[0]


def host_track_es_of(rec, integrity, time=0.0):
    """adsb_host_track_es_of: the AIRCRAFT_ES_DTYPE record of an aircraft whose only counted frame has the ES_DTYPE
    record `rec` and the per-frame output `integrity` (FRAME_INTEGRITY_DTYPE), heard at `time`.  Needs no device."""
    r, f = np.array([rec], dtype=ES_DTYPE), np.array([integrity], dtype=FRAME_INTEGRITY_DTYPE)
    out = np.zeros(1, dtype=AIRCRAFT_ES_DTYPE)
    L.check(L.load().adsb_host_track_es_of(r.ctypes.data, f.ctypes.data, float(time), out.ctypes.data), "adsb_host_track_es_of")
    return out[0]


def host_track_es_merge(into, later):
    """adsb_host_track_es_merge, the combine of an es reserve: the AIRCRAFT_ES_DTYPE record `into` followed by `later`
    -> the merged record.  Needs no device."""
    a, b = np.array([into], dtype=AIRCRAFT_ES_DTYPE), np.array([later], dtype=AIRCRAFT_ES_DTYPE)
    L.check(L.load().adsb_host_track_es_merge(a.ctypes.data, b.ctypes.data), "adsb_host_track_es_merge")
    return a[0]


def host_track_es(frames, es, modes=None, seconds_per_sample=0.5e-6, sample_base=0, max_age_s=60.0, state=None,
                  max_aircraft=None):
    """What a table with an es reserve (and room for every aircraft) makes of ONE list, without a device, from the CPU
    mirror's per-frame functions: FRAME_DTYPE frames with their ES_DTYPE records (and, on the keyed path, their
    MODES_DTYPE records) -> (addresses ascending, their AIRCRAFT_ES_DTYPE records, the per-frame
    FRAME_INTEGRITY_DTYPE output).  state: the dict address -> record a previous call returned through it, carried on
    and updated in place (several updates of one table).  max_aircraft: the table's capacity; as in the table, a call
    admits its new addresses in ascending order while there is room, and the frames of an aircraft it turns away count
    nothing and get an all-zero output."""
    frames = np.ascontiguousarray(frames, dtype=FRAME_DTYPE)
    es = np.ascontiguousarray(es, dtype=ES_DTYPE)
    out = np.zeros(len(frames), dtype=FRAME_INTEGRITY_DTYPE)
    state = {} if state is None else state
    none = np.zeros(1, dtype=ES_DTYPE)[0]
    empty = host_track_es_of(none, np.zeros(1, dtype=FRAME_INTEGRITY_DTYPE)[0])
    keys = [int.from_bytes(frames["bytes"][j][1:4].tobytes(), "big") if modes is None
            else None if int(modes[j]["kind"]) > L.ADSB_MODES_KNOWN else int(modes[j]["address"]) & 0xFFFFFF
            for j in range(len(frames))]
    new = sorted({k for k in keys if k is not None} - set(state))
    for icao in new if max_aircraft is None else new[:max(int(max_aircraft) - len(state), 0)]:
        state[icao] = empty
    for j, icao in enumerate(keys):
        if icao not in state:
            continue
        t = float(int(sample_base) + int(frames["offset"][j])) * seconds_per_sample
        held = state[icao]
        out[j] = host_es_resolve(es[j], t, held, max_age_s)
        state[icao] = host_track_es_merge(held, host_track_es_of(es[j], out[j], t))
    order = sorted(state)
    return (np.array(order, dtype=np.uint32), np.array([state[a] for a in order], dtype=AIRCRAFT_ES_DTYPE).reshape(-1), out)


def aircraft_es_physical(recs):
    """The values of AIRCRAFT_ES_DTYPE records (TrackTable.es) in physical units, the per-aircraft counterpart of
    es_physical with its conversions: a dict of float64 arrays, one entry per aircraft, NaN for what the aircraft has not
    said.  rc_m: the resolved containment radius of its newest position message in metres (NaN: no position message, or
    a radius the table calls unknown); selected_altitude_ft, baro_setting_mb, selected_heading_deg: of its newest
    target state message."""
    recs = np.atleast_1d(np.asarray(recs, dtype=AIRCRAFT_ES_DTYPE))
    out = {"rc_m": np.where(~np.isnan(recs["position_time"]) & (recs["rc_dm"] != 0),
                            recs["rc_dm"] * _ES_PHYSICAL["rc_m"][3], np.nan)}
    held = ~np.isnan(recs["time"][:, 2])
    for key, value in es_physical(recs["target_state"]).items():
        if key != "rc_m":
            out[key] = np.where(held, value, np.nan)
    return out


AIRCRAFT_ES_COLUMNS = ("Ver", "NIC", "Rc", "NACp", "SIL", "Emerg", "Squawk(ES)", "SelAlt")


def aircraft_es_columns(recs):
    """AIRCRAFT_ES_DTYPE records as the text columns AIRCRAFT_ES_COLUMNS, one list of eight strings per aircraft: the
    ADS-B version, NIC and Rc in metres of the newest position message as the table resolved them (a "?" behind NIC
    and Rc where the version was not known when it was heard: Rc is then what the type code alone gives), NACp and SIL
    of the newest operational status (airborne or surface, whichever is newer) or, without one, target state message,
    the emergency state and squawk of the newest TC 28 message, and the selected altitude in feet; "n/a" for what the
    aircraft has not said."""
    recs = np.atleast_1d(np.asarray(recs, dtype=AIRCRAFT_ES_DTYPE))
    p = aircraft_es_physical(recs)
    rows = []
    for k, r in enumerate(recs):
        ver = "n/a" if np.isnan(r["version_time"]) else str(int(r["version"]))
        nic = rc = "n/a"
        if not np.isnan(r["position_time"]):
            mark = "" if int(r["position_supp"]) & L.ADSB_TRACK_ES_VERSIONED << 1 else "?"
            nic = f"{int(r['nic'])}{mark}"
            rc = "n/a" if np.isnan(p["rc_m"][k]) else f"{p['rc_m'][k]:.1f}{mark}"
        times = np.where(np.isnan(r["time"][:3]), -np.inf, r["time"][:3])
        nacp = sil = "n/a"
        for name, t in sorted(zip(AIRCRAFT_ES_BLOCKS[:3], times), key=lambda x: (-x[1], x[0] == "target_state")):
            b = r[name]
            if t > -np.inf and int(b["present"]) & L.ADSB_ES_HAS_NAC_P:
                nacp, sil = str(int(b["nac_p"])), str(int(b["sil"])) if int(b["present"]) & L.ADSB_ES_HAS_SIL else "n/a"
                break
        emerg = squawk = "n/a"
        if not np.isnan(r["time"][3]):
            emerg, squawk = str(int(r["emergency"]["emergency"])), f"{int(r['emergency']['half'][0]):04d}"
        sel = "n/a" if np.isnan(p["selected_altitude_ft"][k]) else f"{p['selected_altitude_ft'][k]:.0f}"
        rows.append([ver, nic, rc, nacp, sil, emerg, squawk, sel])
    return rows


COMMB_SETTLED = L.ADSB_COMMB_SETTLED     # COMMB_DTYPE state of a table's per-frame output: settled by the table
# aircraft_commb_physical: key -> (block, index into value[], what one unit of the value is in the key's unit)
_AIRCRAFT_COMMB_PHYSICAL = {key: ("bds%02x" % bds, k, factor) for key, (bds, k, factor) in _COMMB_PHYSICAL.items()}


def aircraft_commb_physical(recs):
    """The values of AIRCRAFT_COMMB_DTYPE records (TrackTable.commb) in physical units, the per-aircraft counterpart of
    commb_physical: a dict of float64 arrays, one entry per aircraft, NaN for what a block does not hold (no such
    register yet, or its status bit off).  The keys of commb_physical (feet, mb, degrees, kt, Mach, ft/min), and per
    block "bds40_time", "bds50_time", "bds60_time" (NaN = none) and "bds40_settled" ... (1.0 where the block came from
    a reply the table settled, 0.0 where adsb_commb_of found it unambiguous, NaN for none)."""
    recs = np.atleast_1d(np.asarray(recs, dtype=AIRCRAFT_COMMB_DTYPE))
    out = {}
    for key, (block, k, factor) in _AIRCRAFT_COMMB_PHYSICAL.items():
        b = recs[block]
        held = ~np.isnan(b["time"]) & ((b["status"] >> k) & 1 == 1)
        out[key] = np.where(held, b["value"][:, k] * factor, np.nan)
    for block in ("bds40", "bds50", "bds60"):
        b = recs[block]
        out[block + "_time"] = b["time"].astype(np.float64)
        out[block + "_settled"] = np.where(np.isnan(b["time"]), np.nan, b["settled"].astype(np.float64))
    return out


def host_commb_settle(frame_bytes, rec, reference=None, time=0.0, max_age_s=10.0, max_speed_diff_kt=40,
                      max_vrate_diff_fpm=1000):
    """adsb_host_commb_settle, the CPU mirror of a commb reserve's settle: the per-frame output (COMMB_DTYPE) of a
    counted frame with these 14 bytes and stateless record `rec`, heard at `time`, against the VELOCITY_DTYPE record
    `reference` (None: no reference).  Needs no device."""
    b = np.zeros(14, dtype=np.uint8)
    raw = np.frombuffer(bytes(frame_bytes), dtype=np.uint8)[:14]
    b[:len(raw)] = raw
    r = np.array([rec], dtype=COMMB_DTYPE)
    ref = None if reference is None else np.array([reference], dtype=VELOCITY_DTYPE)
    cfg = L.AdsbCommbSettleCfg(float(max_age_s), int(max_speed_diff_kt), int(max_vrate_diff_fpm))
    out = np.zeros(1, dtype=COMMB_DTYPE)
    L.check(L.load().adsb_host_commb_settle(b.ctypes.data, r.ctypes.data, None if ref is None else ref.ctypes.data,
                                            float(time), C.byref(cfg), out.ctypes.data), "adsb_host_commb_settle")
    return out[0]


def host_commb_reference(frame_bytes, time=0.0):
    """adsb_host_commb_reference: the VELOCITY_DTYPE record, exact fields only, that a table reads as the reference from
    a DF17/18 TC 19 frame of the current list (subtype 0: ST 0 and 5-7 are none).  Needs no device."""
    b = np.zeros(14, dtype=np.uint8)
    raw = np.frombuffer(bytes(frame_bytes), dtype=np.uint8)[:14]
    b[:len(raw)] = raw
    out = np.zeros(1, dtype=VELOCITY_DTYPE)
    L.check(L.load().adsb_host_commb_reference(b.ctypes.data, float(time), out.ctypes.data), "adsb_host_commb_reference")
    return out[0]


def host_track_commb_of(rec, time=0.0):
    """adsb_host_track_commb_of: the AIRCRAFT_COMMB_DTYPE record of an aircraft whose only counted frame has the
    per-frame output `rec` (COMMB_DTYPE), heard at `time`.  Needs no device."""
    r = np.array([rec], dtype=COMMB_DTYPE)
    out = np.zeros(1, dtype=AIRCRAFT_COMMB_DTYPE)
    L.check(L.load().adsb_host_track_commb_of(r.ctypes.data, float(time),
                                              out.ctypes.data_as(C.POINTER(L.AdsbAircraftCommb))),
            "adsb_host_track_commb_of")
    return out[0]


def host_track_commb_merge(into, later):
    """adsb_host_track_commb_merge, the combine of a commb reserve: the AIRCRAFT_COMMB_DTYPE record `into` followed by
    `later` -> the merged record.  Needs no device."""
    a, b = np.array([into], dtype=AIRCRAFT_COMMB_DTYPE), np.array([later], dtype=AIRCRAFT_COMMB_DTYPE)
    P = C.POINTER(L.AdsbAircraftCommb)
    L.check(L.load().adsb_host_track_commb_merge(a.ctypes.data_as(P), b.ctypes.data_as(P)), "adsb_host_track_commb_merge")
    return a[0]


def host_track_commb(frames, modes, commb, seconds_per_sample=0.5e-6, sample_base=0, **limits):
    """What a table with a modes and a commb reserve (and room for every aircraft) makes of ONE list, without a device,
    from the CPU mirror's per-frame functions: FRAME_DTYPE frames with their MODES_DTYPE and COMMB_DTYPE records ->
    (addresses ascending, their AIRCRAFT_COMMB_DTYPE records, the per-frame COMMB_DTYPE output).  limits: commb_reserve's."""
    frames = np.ascontiguousarray(frames, dtype=FRAME_DTYPE)
    out, state, held = np.array(commb, dtype=COMMB_DTYPE), {}, {}
    for j in range(len(frames)):
        if int(modes[j]["kind"]) > L.ADSB_MODES_KNOWN:
            continue
        icao, b = int(modes[j]["address"]) & 0xFFFFFF, frames["bytes"][j].tobytes()
        t = float(int(sample_base) + int(frames["offset"][j])) * seconds_per_sample
        if icao not in state:
            state[icao] = host_track_commb_of(np.zeros(1, dtype=COMMB_DTYPE)[0])
        if int(commb[j]["state"]) != L.ADSB_COMMB_NOT_COMMB:
            out[j] = host_commb_settle(b, commb[j], held.get(icao), t, **limits)
            state[icao] = host_track_commb_merge(state[icao], host_track_commb_of(out[j], t))
        if int(modes[j]["df"]) in (17, 18) and b[4] >> 3 == 19:
            v = host_commb_reference(b, t)
            if int(v["subtype"]):
                held[icao] = v
    order = sorted(state)
    return (np.array(order, dtype=np.uint32), np.array([state[a] for a in order], dtype=AIRCRAFT_COMMB_DTYPE).reshape(-1), out)


AIRCRAFT_COMMB_COLUMNS = ("SelAlt", "QNH", "GS/Trk(B)", "Hdg", "IAS", "Mach")


def aircraft_commb_columns(recs):
    """AIRCRAFT_COMMB_DTYPE records as the text columns AIRCRAFT_COMMB_COLUMNS, one list of six strings per aircraft:
    selected altitude in feet (MCP/FCU, else FMS), barometric setting in mb, ground speed in kt / true track in degrees
    from BDS 5,0, magnetic heading, IAS and Mach from BDS 6,0; "n/a" for what the aircraft has not said, and a "*" behind
    a value from a reply the table settled (it read as 5,0 and as 6,0; the aircraft's ADS-B velocity decided)."""
    p = aircraft_commb_physical(recs)
    rows = []
    for k in range(len(p["mach"])):
        f = lambda key, fmt: "n/a" if np.isnan(p[key][k]) else format(p[key][k], fmt)
        m5 = "*" if p["bds50_settled"][k] == 1.0 else ""
        m6 = "*" if p["bds60_settled"][k] == 1.0 else ""
        sel = f("mcp_altitude_ft", ".0f") if not np.isnan(p["mcp_altitude_ft"][k]) else f("fms_altitude_ft", ".0f")
        gs_trk = f("ground_speed_kt", ".0f") + "/" + f("true_track_deg", ".0f")
        rows.append([sel, f("baro_setting_mb", ".1f"), "n/a" if gs_trk == "n/a/n/a" else gs_trk + m5,
                     f("magnetic_heading_deg", ".0f") + (m6 if not np.isnan(p["magnetic_heading_deg"][k]) else ""),
                     f("ias_kt", ".0f") + (m6 if not np.isnan(p["ias_kt"][k]) else ""),
                     f("mach", ".3f") + (m6 if not np.isnan(p["mach"][k]) else "")])
    return rows


MESSAGE_DTYPE = np.dtype([("time", "<u8"), ("bytes", "u1", (14,)), ("status", "u1"), ("fixed_bit", "u1"), ("first", "<u4"),
                          ("n_receptions", "<u4"), ("n_receivers", "<u2"), ("first_receiver", "<u2"),
                          ("best_receiver", "<u2"), ("reserved", "<u2"), ("n_clean", "<u4"), ("reserved2", "<u4"),
                          ("span", "<u8"), ("best_signal_sum", "<u8")])
assert MESSAGE_DTYPE.itemsize == C.sizeof(L.AdsbMessage) == 64
RECEPTION_DTYPE = np.dtype([("time", "<u8"), ("frame", "<u4"), ("receiver", "<u2"), ("reserved", "<u2")])
assert RECEPTION_DTYPE.itemsize == C.sizeof(L.AdsbReception) == 16


def _u64_list(values, n, what):
    """(array kept alive, pointer or None) of n uint64 values (None: a NULL pointer)."""
    if values is None:
        return None, None
    arr = np.ascontiguousarray(values, dtype=np.uint64).reshape(-1)
    if len(arr) != n:
        raise ValueError(f"{what}: {len(arr)} values for {n} receivers")
    return arr, arr.ctypes.data


def frames_of_messages(messages):
    """Bytes 0..23 of every MESSAGE_DTYPE record as a FRAME_DTYPE list (offset = time): what the device also writes
    contiguously as frames_out."""
    messages = np.ascontiguousarray(messages, dtype=MESSAGE_DTYPE)
    out = np.zeros(len(messages), dtype=FRAME_DTYPE)
    out["offset"], out["bytes"] = messages["time"], messages["bytes"]
    out["status"], out["fixed_bit"] = messages["status"], messages["fixed_bit"]
    return out


def host_correlate(frames, counts, window, sample_base=None, levels=None):
    """adsb_host_correlate, the CPU mirror of AdsbDemod.correlate_of: (messages, frames, receptions) as MESSAGE_DTYPE,
    FRAME_DTYPE and RECEPTION_DTYPE arrays of the multi-receiver FRAME_DTYPE list `frames` (receiver 0's frames, then
    receiver 1's, ...; counts[r] frames each), with sample_base[r] added to receiver r's offsets and the frames'
    LEVEL_DTYPE records `levels` (None: no best receiver).  window: samples.  Needs no device."""
    frames, fptr, n = _host_list(frames, FRAME_DTYPE)
    lptr = None
    if levels is not None:
        levels, lptr, _ = _host_list(levels, LEVEL_DTYPE, n)
    counts = np.ascontiguousarray(counts, dtype=np.uint64).reshape(-1)
    base, bptr = _u64_list(sample_base, len(counts), "sample_base")
    cfg = L.AdsbCorrelateCfg(int(window), 0, 0)
    msgs = np.zeros(max(n, 1), dtype=MESSAGE_DTYPE)
    fout = np.zeros(max(n, 1), dtype=FRAME_DTYPE)
    recs = np.zeros(max(n, 1), dtype=RECEPTION_DTYPE)
    n_msgs = C.c_size_t()
    L.check(L.load().adsb_host_correlate(C.byref(cfg), fptr, lptr, n, counts.ctypes.data if len(counts) else None,
                                         len(counts), bptr, msgs.ctypes.data, n, C.byref(n_msgs), fout.ctypes.data,
                                         recs.ctypes.data), "adsb_host_correlate")
    return msgs[:n_msgs.value].copy(), fout[:n_msgs.value].copy(), recs[:n].copy()


MLAT_FIX_DTYPE, MLAT_RECEIVER_DTYPE = L.MLAT_FIX_DTYPE, L.MLAT_RECEIVER_DTYPE
MLAT_HEADER_DTYPE = np.dtype([(k, "<u8") for k in ("n_messages", "n_attempted", "n_valid", "flags")])
assert MLAT_HEADER_DTYPE.itemsize == C.sizeof(L.AdsbMlatHeader) == 32
MLAT_TIME_SOURCES = {"reception": L.ADSB_MLAT_TIME_RECEPTION, "ticks": L.ADSB_MLAT_TIME_TICKS}


def _mlat_cfg(time_source="reception", seconds_per_tick=0.0, use_altitude=False, min_receivers=0, max_iterations=0,
              step_tol_m=0.0, max_residual_m=0.0, max_range_m=0.0, default_altitude_m=0.0):
    src = MLAT_TIME_SOURCES[time_source] if isinstance(time_source, str) else int(time_source)
    return L.AdsbMlatCfg(src, L.ADSB_MLAT_USE_ALTITUDE if use_altitude else 0, int(min_receivers), int(max_iterations),
                         float(seconds_per_tick), float(step_tol_m), float(max_residual_m), float(max_range_m),
                         float(default_altitude_m), 0)


def _mlat_receivers(receivers):
    """An MLAT_RECEIVER_DTYPE array of such an array or of (latitude, longitude, height_m[, clock_offset_s = 0])
    tuples."""
    if isinstance(receivers, np.ndarray) and receivers.dtype == MLAT_RECEIVER_DTYPE:
        return np.ascontiguousarray(receivers).reshape(-1)
    out = np.zeros(len(receivers), dtype=MLAT_RECEIVER_DTYPE)
    for k, r in enumerate(receivers):
        r = tuple(r)
        out[k] = (r[0], r[1], r[2], r[3] if len(r) > 3 else 0.0)
    return out


def _mlat_list(arr, dtype):
    """(kept alive, pointer or None, count) of a host array, None, or a (device pointer, count) pair."""
    if arr is None:
        return None, None, 0
    if isinstance(arr, tuple):
        return None, (int(arr[0]) if arr[1] else None), int(arr[1])
    return _host_list(arr, dtype)


def host_multilaterate(receivers, messages, receptions, rx=None, **cfg):
    """adsb_host_multilaterate, the CPU mirror of AdsbDemod.multilaterate_of: (MLAT_FIX_DTYPE fixes, one per message;
    the MLAT_HEADER_DTYPE record) of a correlate result (MESSAGE_DTYPE, RECEPTION_DTYPE) heard by `receivers`
    (MLAT_RECEIVER_DTYPE, or (latitude, longitude, height_m[, clock_offset_s]) tuples).  rx: the WIRE_RX_DTYPE records of
    the correlated list, for time_source="ticks".  Keywords: time_source ("reception" / "ticks"), seconds_per_tick,
    use_altitude, min_receivers, max_iterations, step_tol_m, max_residual_m, max_range_m, default_altitude_m; 0 takes
    each default.  Needs no device."""
    rcv = _mlat_receivers(receivers)
    c = _mlat_cfg(**cfg)
    msgs, mptr, nm = _host_list(messages, MESSAGE_DTYPE)
    recs, rptr, nr = _host_list(receptions, RECEPTION_DTYPE)
    rxa, xptr, nx = _mlat_list(rx, WIRE_RX_DTYPE)
    fixes = np.zeros(max(nm, 1), dtype=MLAT_FIX_DTYPE)
    hdr = L.AdsbMlatHeader()
    L.check(L.load().adsb_host_multilaterate(C.byref(c), rcv.ctypes.data if len(rcv) else None, len(rcv), mptr, nm, rptr,
                                             nr, xptr, nx, fixes.ctypes.data, C.byref(hdr)), "adsb_host_multilaterate")
    return fixes[:nm].copy(), np.frombuffer(bytes(hdr), dtype=MLAT_HEADER_DTYPE)[0]


CLOCK_DTYPE = L.CLOCK_DTYPE
CLOCK_HEADER_DTYPE = np.dtype([(k, "<u8") for k in ("n_messages", "n_eligible", "n_rows", "n_dropped", "n_reached",
                                                    "flags")] + [("reserved", "<u8", (2,))])
assert CLOCK_HEADER_DTYPE.itemsize == C.sizeof(L.AdsbClockHeader) == 64


def _clock_cfg(time_source="reception", seconds_per_tick=0.0, seconds_per_time=0.0, reference=0, drift=True, min_rows=0,
               max_residual_s=0.0, max_range_nm=0.0):
    src = MLAT_TIME_SOURCES[time_source] if isinstance(time_source, str) else int(time_source)
    return L.AdsbClockCfg(src, L.ADSB_CLOCK_DRIFT if drift else 0, int(reference), int(min_rows), float(seconds_per_tick),
                          float(seconds_per_time), float(max_residual_s), float(max_range_nm))


def host_clock_sync(receivers, messages, receptions, rx=None, row_state=False, **cfg):
    """adsb_host_clock_sync, the CPU mirror of AdsbDemod.clock_sync_of: (CLOCK_DTYPE clocks, one per receiver; the
    CLOCK_HEADER_DTYPE record[; one byte per reception slot: 0 empty, 1 a kept row, 2 a dropped row]) of a correlate
    result heard by `receivers`, whose clock_offset_s is the prior.  Keywords: time_source ("reception" / "ticks"),
    seconds_per_tick, seconds_per_time (the unit of the messages' time), reference, drift (solve one per receiver),
    min_rows, max_residual_s (> 0: a second pass without the rows beyond it), max_range_nm.  Needs no device."""
    rcv = _mlat_receivers(receivers)
    c = _clock_cfg(**cfg)
    msgs, mptr, nm = _host_list(messages, MESSAGE_DTYPE)
    recs, rptr, nr = _host_list(receptions, RECEPTION_DTYPE)
    rxa, xptr, nx = _mlat_list(rx, WIRE_RX_DTYPE)
    clocks = np.zeros(max(len(rcv), 1), dtype=CLOCK_DTYPE)
    state = np.zeros(max(nr, 1), dtype=np.uint8)
    hdr = L.AdsbClockHeader()
    L.check(L.load().adsb_host_clock_sync(C.byref(c), rcv.ctypes.data if len(rcv) else None, len(rcv), mptr, nm, rptr,
                                          nr, xptr, nx, clocks.ctypes.data, C.byref(hdr), state.ctypes.data),
            "adsb_host_clock_sync")
    out = (clocks[:len(rcv)].copy(), np.frombuffer(bytes(hdr), dtype=CLOCK_HEADER_DTYPE)[0])
    return out + (state[:nr].copy(),) if row_state else out


def host_clock_apply(clocks, messages, receptions, rx=None, **cfg):
    """adsb_host_clock_apply, the CPU mirror of AdsbDemod.clock_apply: the RECEPTION_DTYPE list with corrected times, in
    units of seconds_per_tick / 256.  cfg: the keywords of the sync."""
    clocks = np.ascontiguousarray(clocks, dtype=CLOCK_DTYPE)
    c = _clock_cfg(**cfg)
    msgs, mptr, nm = _host_list(messages, MESSAGE_DTYPE)
    recs, rptr, nr = _host_list(receptions, RECEPTION_DTYPE)
    rxa, xptr, nx = _mlat_list(rx, WIRE_RX_DTYPE)
    out = np.zeros(max(nr, 1), dtype=RECEPTION_DTYPE)
    L.check(L.load().adsb_host_clock_apply(C.byref(c), clocks.ctypes.data if len(clocks) else None, len(clocks), mptr, nm,
                                           rptr, nr, xptr, nx, out.ctypes.data), "adsb_host_clock_apply")
    return out[:nr].copy()


def level_dbfs(sample_type, total, n_samples):
    """adsb_level_dbfs: 10 log10(total / n_samples / full scale) -- a LEVEL_DTYPE sum as mean power in dBFS (-inf for
    0).  level_dbfs(st, rec["signal_sum"], LEVEL_PULSE_SAMPLES), level_dbfs(st, rec["noise_sum"], LEVEL_QUIET_SAMPLES)."""
    return float(L.load().adsb_level_dbfs(int(sample_type), int(total), int(n_samples)))


def measure_feed(device, sample_type, chunk, seconds=0.15):
    """(us per buffer, frames per buffer, buffers) of the streaming front end fed from pinned HOST memory, timed in C."""
    us, fr, nb = C.c_double(), C.c_double(), C.c_uint64()
    L.check(L.load().adsb_measure_feed(int(device), int(sample_type), int(chunk), float(seconds), C.byref(us), C.byref(fr),
                                       C.byref(nb)), "adsb_measure_feed")
    return us.value, fr.value, nb.value


def measure_pinned_copy(device, nbytes=64 << 20, iters=8):
    """Pinned host -> device copy rate of this box in GB/s."""
    g = C.c_double()
    L.check(L.load().adsb_measure_pinned_copy(int(device), int(nbytes), int(iters), C.byref(g)), "adsb_measure_pinned_copy")
    return g.value


def synth_slot(cfg, channel, slot):
    start = C.c_uint64()
    clean = (C.c_uint8 * 14)()
    sent = (C.c_uint8 * 14)()
    kind = C.c_int()
    r = L.load().adsb_synth_slot(C.byref(cfg), channel, slot, C.byref(start), C.byref(clean),
                                 C.byref(sent), C.byref(kind))
    if r < 0:
        raise L.AdsbError(r, "adsb_synth_slot")
    return bool(r), start.value, bytes(clean), bytes(sent), kind.value


TRACK_POINT_DTYPE = np.dtype([("latitude", "<f8"), ("longitude", "<f8"), ("icao", "<u4"), ("flags", "<u4")])
AIRCRAFT_DTYPE = np.dtype([("latitude", "<f8"), ("longitude", "<f8"), ("last_contact", "<f8"), ("icao", "<u4"),
                           ("altitude", "<i4"), ("has_position", "<u4"), ("n_frames", "<u4"), ("callsign", "S8")])
VELOCITY_DTYPE = np.dtype([("time", "<f8"), ("speed_kt", "<f4"), ("direction_deg", "<f4"),
                           ("vertical_rate_fpm", "<i4"), ("v_ew_kt", "<i2"), ("v_ns_kt", "<i2"), ("subtype", "u1"),
                           ("flags", "u1"), ("vrate_baro", "u1"), ("airspeed_tas", "u1"), ("reserved", "<u4")])
assert VELOCITY_DTYPE.itemsize == C.sizeof(L.AdsbVelocity) == 32
FUSED_DTYPE = np.dtype([("latitude", "<f8"), ("longitude", "<f8"), ("position_time", "<f8"), ("last_contact", "<f8"),
                        ("last_heard", "<f8"), ("n_frames", "<u8"), ("icao", "<u4"), ("altitude", "<i4"),
                        ("n_receivers", "<u2"), ("heard_receiver", "<u2"), ("contact_receiver", "<u2"),
                        ("position_receiver", "<u2"), ("callsign_receiver", "<u2"), ("velocity_receiver", "<u2"),
                        ("has_position", "<u4"), ("callsign", "S8"), ("velocity", VELOCITY_DTYPE),
                        ("reserved", "<u8", (2,))])
assert FUSED_DTYPE.itemsize == C.sizeof(L.AdsbFusedAircraft) == 128
AIRCRAFT_LEVEL_DTYPE = np.dtype([("signal_total", "<u8"), ("noise_total", "<u8"), ("last_signal_sum", "<u8"),
                                 ("last_noise_sum", "<u8"), ("max_signal_sum", "<u8"), ("last_time", "<f8"),
                                 ("n_levels", "<u4"), ("peak", "<u4"), ("weak_bits_total", "<u4"), ("reserved", "<u4")])
assert AIRCRAFT_LEVEL_DTYPE.itemsize == C.sizeof(L.AdsbAircraftLevel) == 64
FUSED_LEVEL_DTYPE = np.dtype([("strongest", AIRCRAFT_LEVEL_DTYPE), ("signal_total", "<u8"), ("noise_total", "<u8"),
                              ("n_levels", "<u8"), ("strongest_receiver", "<u2"), ("level_receivers", "<u2"),
                              ("reserved", "<u4")])
assert FUSED_LEVEL_DTYPE.itemsize == C.sizeof(L.AdsbFusedLevel) == 96


class Tracker:
    """Host mirror of the reference's `HashMap<u32, Aircraft>` + handle_aircraft_update (aircraft.rs:158-165)."""

    def __init__(self):
        self._lib = L.load()
        self._h = self._lib.adsb_tracker_create()

    def update(self, frame_bytes, time_s):
        b = np.frombuffer(bytes(frame_bytes), dtype=np.uint8).copy()
        out = L.AdsbAircraftSummary()
        r = self._lib.adsb_tracker_update(self._h, b.ctypes.data, float(time_s), C.byref(out))
        if r < 0:
            raise L.AdsbError(r, "adsb_tracker_update")
        return bool(r), out

    def get(self, icao):
        out = L.AdsbAircraftSummary()
        L.check(self._lib.adsb_tracker_get(self._h, icao, C.byref(out)), "adsb_tracker_get")
        return out

    def __len__(self):
        return self._lib.adsb_tracker_count(self._h)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.adsb_tracker_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def cpr_position(even_lat, even_lon, odd_lat, odd_lon, first_is_odd):
    """cpr.rs:135-147 through the host mirror: (lat, lon) or None."""
    lib = L.load()
    lat, lon = C.c_double(), C.c_double()
    r = lib.adsb_cpr_position(even_lat, even_lon, odd_lat, odd_lon, int(first_is_odd), C.byref(lat), C.byref(lon))
    return (lat.value, lon.value) if r == 1 else None


class AdsbDemod:
    """adsb_ctx wrapper.  ``stream`` is a hipStream_t as int (e.g. torch's current stream)."""

    def __init__(self, device=0, sample_type=L.ADSB_SAMPLE_I8, max_samples=1 << 20, max_out=1 << 16,
                 max_channels=1, stream=None, host_staging=True):
        self._lib = L.load()
        cfg = L.AdsbCfg(L.ADSB_ABI_VERSION, device, sample_type, max_channels, max_samples, max_out,
                        stream, 1 if host_staging else 0, 0)
        h = C.c_void_p()
        L.check(self._lib.adsb_create(C.byref(cfg), C.byref(h)), "adsb_create")
        self._h = h
        self.device = device
        self.sample_type = sample_type
        self.max_out = max_out
        self.max_channels = max_channels
        self._last_channels = 1   # channels of the last launch (adsb_demod is single-channel)
        self._np_dtype = np.int8 if sample_type == L.ADSB_SAMPLE_I8 else np.int16

    def close(self):
        if getattr(self, "_h", None):
            self._lib.adsb_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    @property
    def stream(self):
        return self._lib.adsb_stream(self._h)

    @property
    def mag_mode(self):
        return self._lib.adsb_debug_mag_mode(self._h)

    @property
    def scan(self):
        """Which scan kernel this context launches (fixed at adsb_create by ADSB_SCAN): 'root' (floor(sqrt) per sample, u8
        magnitudes in LDS: the product's, the default; CS16's only one), or one of the A/B kernels of rounds 3-4, in
        -DADSB_AB_KERNELS=1 builds only: 'nsq', 'reg', 'code', 'sieve' (DESIGN.md sections 4.1b-d)."""
        return {0: "nsq", 1: "root", 2: "reg", 3: "code", 4: "sieve"}[self._lib.adsb_debug_scan(self._h)]

    def code_table(self):
        """The code scan's table as the device computes it: uint16[32769], c(n) | th(n) << 8."""
        out = np.empty(32769, dtype=np.uint16)
        L.check(self._lib.adsb_debug_code_table(self._h, out.ctypes.data), "adsb_debug_code_table")
        return out

    def set_launch_index(self, idx):
        """Test knob: the next launch counts as launch number idx (epoch of finish_order's exchange words)."""
        L.check(self._lib.adsb_debug_set_launch_index(self._h, int(idx) & 0xFFFFFFFF), "adsb_debug_set_launch_index")

    def finish_stall(self, blk=0xFFFFFFFF):
        """Test knob: finish_order's workgroup blk withholds its exchange word (default: none does)."""
        L.check(self._lib.adsb_debug_finish_stall(self._h, int(blk) & 0xFFFFFFFF), "adsb_debug_finish_stall")

    def pool_limit(self, on=True):
        """Test knob: the shared slot pool hands out nothing (tiles over their quota lose their slots)."""
        L.check(self._lib.adsb_debug_pool_limit(self._h, 1 if on else 0), "adsb_debug_pool_limit")

    # -- behind the channel: tracker + CPR on the device (aircraft.rs, cpr.rs) ------------------------
    def track(self, seconds_per_sample=0.5e-6):
        """Runs the tracker over the last (single-channel) launch's frame list.  Returns (points, aircraft):
        structured arrays, one point per frame (frame order) and one record per ICAO (ascending)."""
        L.check(self._lib.adsb_track_device(self._h, float(seconds_per_sample)), "adsb_track_device")
        pts = np.zeros(max(self.max_out, 1), dtype=TRACK_POINT_DTYPE)
        acs = np.zeros(max(self.max_out, 1), dtype=AIRCRAFT_DTYPE)
        npts, nac = C.c_size_t(), C.c_size_t()
        L.check(self._lib.adsb_fetch_track(self._h, pts.ctypes.data, len(pts), C.byref(npts), acs.ctypes.data,
                                           len(acs), C.byref(nac)), "adsb_fetch_track")
        return pts[:npts.value].copy(), acs[:min(nac.value, len(acs))].copy()

    def fused_pass_only(self, on=True):
        """Measurement only: following launches stop after the fused magnitude + gate pass (no frames)."""
        L.check(self._lib.adsb_debug_fused_pass_only(self._h, 1 if on else 0), "adsb_debug_fused_pass_only")

    def tile_stamps(self, max_tiles=1 << 20):
        """Diagnostic builds (-DADSB_TILE_STAMPS=1): (n_tiles, 16) uint32 of the last launch."""
        out = np.zeros((max_tiles, 16), dtype=np.uint32)
        n = C.c_size_t()
        L.check(self._lib.adsb_debug_tile_stamps(self._h, out.ctypes.data, max_tiles, C.byref(n)), "adsb_debug_tile_stamps")
        return out[:n.value].copy()

    # -- one received buffer (reference adsb.rs:95-116) -------------------------------------------
    def demod(self, iq, max_out=None):
        """iq: array of shape (n, 2) [I, Q] of the ctx sample dtype.  Returns (frames, flags)."""
        iq = np.ascontiguousarray(iq, dtype=self._np_dtype)
        n = iq.shape[0] if iq.ndim == 2 else iq.size // 2
        cap = self.max_out if max_out is None else max_out
        out = np.zeros(max(cap, 1), dtype=FRAME_DTYPE)
        n_out = C.c_size_t()
        flags = C.c_uint32()
        L.check(self._lib.adsb_demod(self._h, iq.ctypes.data, n,
                                     out.ctypes.data_as(C.POINTER(L.AdsbFrame)), cap, C.byref(n_out),
                                     C.byref(flags)), "adsb_demod")
        self._last_channels = 1
        return out[:n_out.value].copy(), flags.value

    # -- HBM-resident, asynchronous -----------------------------------------------------------------
    def demod_device_async(self, dev_ptr, n_samples, n_channels=1, channel_stride=None):
        stride = n_samples if channel_stride is None else channel_stride
        L.check(self._lib.adsb_demod_device_async(self._h, dev_ptr, n_channels, n_samples, stride),
                "adsb_demod_device_async")
        self._last_channels = int(n_channels)

    def fetch(self, max_out=None, n_channels=None):
        """Frames of the last launch: (frames, per-channel counts, total_found, flags).  adsb_fetch writes one
        count per channel of the LAST LAUNCH, so the array handed to it always holds max_channels entries; the
        first `n_channels` (default: the last launch's) are returned."""
        cap = self.max_out if max_out is None else max_out
        out = np.zeros(max(cap, 1), dtype=FRAME_DTYPE)
        n_out = C.c_size_t()
        total = C.c_uint64()
        flags = C.c_uint32()
        counts = (C.c_uint64 * max(self.max_channels, 1))()
        L.check(self._lib.adsb_fetch(self._h, out.ctypes.data_as(C.POINTER(L.AdsbFrame)), cap,
                                     C.byref(n_out), counts, C.byref(total), C.byref(flags)),
                "adsb_fetch")
        n = self._last_channels if n_channels is None else min(int(n_channels), self.max_channels)
        return out[:n_out.value].copy(), list(counts)[:n], total.value, flags.value

    def fetch_counts(self):
        n_out, total, flags = C.c_uint64(), C.c_uint64(), C.c_uint32()
        L.check(self._lib.adsb_fetch_counts(self._h, C.byref(n_out), C.byref(total), C.byref(flags)),
                "adsb_fetch_counts")
        return n_out.value, total.value, flags.value

    def result_device(self):
        frames, hdr = C.c_void_p(), C.c_void_p()
        L.check(self._lib.adsb_result_device(self._h, C.byref(frames), C.byref(hdr)),
                "adsb_result_device")
        return frames.value, hdr.value

    def decode_fields(self, max_out=None):
        """On-device AdsbPacket field decode of the last launch's frames -> structured array."""
        L.check(self._lib.adsb_decode_fields_device_async(self._h), "adsb_decode_fields_device_async")
        cap = self.max_out if max_out is None else max_out
        out = np.zeros(max(cap, 1), dtype=FIELDS_DTYPE)
        n = C.c_size_t()
        L.check(self._lib.adsb_fetch_fields(self._h, out.ctypes.data, cap, C.byref(n)), "adsb_fetch_fields")
        return out[:n.value].copy()

    def levels_async(self):
        """adsb_levels_device_async alone: enqueues the last launch's per-frame power statistics and returns."""
        L.check(self._lib.adsb_levels_device_async(self._h), "adsb_levels_device_async")

    def levels(self, max_out=None):
        """Per-frame signal and noise power of the last launch's frames, on the device -> LEVEL_DTYPE array in frame
        order.  Enqueues the kernel first unless levels_async() already did for this launch."""
        cap = self.max_out if max_out is None else max_out
        out = np.zeros(max(cap, 1), dtype=LEVEL_DTYPE)
        n = C.c_size_t()
        ptr = out.ctypes.data_as(C.POINTER(L.AdsbFrameLevel))
        rc = self._lib.adsb_fetch_levels(self._h, ptr, cap, C.byref(n))
        if rc == L.ADSB_E_STATE:               # not enqueued for this launch yet
            self.levels_async()
            rc = self._lib.adsb_fetch_levels(self._h, ptr, cap, C.byref(n))
        L.check(rc, "adsb_fetch_levels")
        return out[:n.value].copy()

    def levels_device(self):
        """Device address of the records levels_async() fills; valid on the ctx stream, no synchronisation."""
        dev = C.c_void_p()
        L.check(self._lib.adsb_levels_device(self._h, C.byref(dev)), "adsb_levels_device")
        return dev.value

    def levels_of(self, dev_ptr, n_samples, frames, first_sample=0):
        """adsb_levels_of: LEVEL_DTYPE records of any frame list against n_samples samples of the ctx's sample type at
        dev_ptr (one channel, device memory) whose sample 0 is stream sample first_sample.  frames: a FRAME_DTYPE array
        (host), or (device pointer, count).  Blocking; the last launch's levels stay as they are."""
        if isinstance(frames, tuple):
            ptr, n = int(frames[0]), int(frames[1])
        else:
            frames = np.ascontiguousarray(frames, dtype=FRAME_DTYPE)
            ptr, n = (frames.ctypes.data if len(frames) else None), len(frames)
        out = np.zeros(max(n, 1), dtype=LEVEL_DTYPE)
        L.check(self._lib.adsb_levels_of(self._h, dev_ptr, int(n_samples), int(first_sample), ptr, n,
                                         out.ctypes.data_as(C.POINTER(L.AdsbFrameLevel))), "adsb_levels_of")
        return out[:n].copy()

    def levels_modes_of(self, dev_ptr, n_samples, frames, counts=None, channel_stride=None, first_sample=0, fetch=True):
        """adsb_levels_modes_of: LEVEL_DTYPE records by frame length of what replies_of / merge_lists produce -- 56-bit
        frames over their 128 samples (ADSB_LEVEL_VALID | ADSB_LEVEL_SHORT), 112-bit frames as levels_of -- against
        len(counts) channels of n_samples samples at dev_ptr, channel_stride samples apart (default n_samples).
        frames: a FRAME_DTYPE array (host), or (device pointer, count), in channel order; counts: frames per channel
        (host; None: one channel).  fetch=False leaves the records on the device: levels_modes_device() is their
        address, which wire_of, correlate_of and a table's update(levels=) take.  Blocking; the last launch's levels
        and levels_of's scratch stay as they are."""
        if isinstance(frames, tuple):
            ptr, n = int(frames[0]), int(frames[1])
        else:
            frames = np.ascontiguousarray(frames, dtype=FRAME_DTYPE)
            ptr, n = (frames.ctypes.data if len(frames) else None), len(frames)
        counts = _channel_counts(counts, n)
        stride = n_samples if channel_stride is None else channel_stride
        out = np.zeros(max(n, 1), dtype=LEVEL_DTYPE) if fetch else None
        L.check(self._lib.adsb_levels_modes_of(self._h, dev_ptr, len(counts), int(n_samples), int(stride),
                                               int(first_sample), ptr, counts.ctypes.data if len(counts) else None, n,
                                               out.ctypes.data if fetch else None), "adsb_levels_modes_of")
        return out[:n].copy() if fetch else None

    def levels_modes_device(self):
        """Device address of the records of the last levels_modes_of(); valid until the next one."""
        dev = C.c_void_p()
        L.check(self._lib.adsb_levels_modes_device(self._h, C.byref(dev)), "adsb_levels_modes_device")
        return dev.value

    def wire_async(self, format="beast", signal=True, tick_bias=0, short=False):
        """adsb_wire_device_async alone: enqueues the last launch's list as Beast binary ("beast") or AVR text ("avr",
        "avr_mlat") behind its ordering pass and returns.  signal: Beast's signal byte from the launch's levels, which
        are enqueued here if they have not been.  Timestamp = 6 x offset + tick_bias, mod 2^48.  short:
        ADSB_WIRE_SHORT (the demodulator's list is all DF17, so its bytes are the same)."""
        cfg = _wire_cfg(format, signal, tick_bias, short)
        L.check(self._lib.adsb_wire_device_async(self._h, C.byref(cfg)), "adsb_wire_device_async")

    def wire(self, format="beast", signal=True, tick_bias=0, short=False):
        """The last launch's frames as one stream: (bytes, ends), ends[i] the exclusive end of frame i's bytes (uint32).
        Encoded on the device; a second call with another format replaces the first's stream."""
        self.wire_async(format, signal, tick_bias, short)
        return self.fetch_wire()

    def fetch_wire(self, cap=None, max_ends=None):
        """adsb_fetch_wire: waits for the stream wire_async() enqueued -> (bytes, ends).  cap / max_ends (default: what
        the stream needs): room for bytes and ends; with less room, whole frames only."""
        total, n = C.c_size_t(), C.c_size_t()
        if cap is None or max_ends is None:      # the sizes first; the stream stays where it is
            L.check(self._lib.adsb_fetch_wire(self._h, None, 0, C.byref(total), None, 0, C.byref(n)), "adsb_fetch_wire")
        room = total.value if cap is None else int(cap)
        n_ends = n.value if max_ends is None else int(max_ends)
        out = np.zeros(max(room, 1), dtype=np.uint8)
        ends = np.zeros(max(n_ends, 1), dtype=np.uint32)
        L.check(self._lib.adsb_fetch_wire(self._h, out.ctypes.data, room, C.byref(total), ends.ctypes.data, n_ends,
                                          C.byref(n)), "adsb_fetch_wire")
        ends = ends[:min(n_ends, n.value)].copy()
        if total.value <= room:
            return out[:total.value].tobytes(), ends
        all_ends = ends if len(ends) == n.value else self.fetch_wire(cap=0)[1]
        return _wire_result(out, room, all_ends, total.value)[0], ends

    def wire_device(self):
        """adsb_wire_device: device addresses (stream, ends, {u64 n_bytes, u64 n_frames}); no synchronisation."""
        b, e, h = C.c_void_p(), C.c_void_p(), C.c_void_p()
        L.check(self._lib.adsb_wire_device(self._h, C.byref(b), C.byref(e), C.byref(h)), "adsb_wire_device")
        return b.value, e.value, h.value

    def wire_of(self, frames, levels=None, format="beast", tick_bias=0, cap=None, short=False):
        """adsb_wire_of: any frame list with any level list as one stream -> (bytes, ends).  frames: a FRAME_DTYPE array
        (host) or (device pointer, count); levels: None (signal byte 0), a LEVEL_DTYPE array (host) or a device pointer.
        cap: room for the bytes (default: enough); with less, whole frames only.  short: ADSB_WIRE_SHORT, 56-bit
        frames leave as short frames and ADSB_LEVEL_SHORT records scale by 60 pulse samples.  Blocking; the last
        launch's wire output stays as it is."""
        if isinstance(frames, tuple):
            fptr, n = int(frames[0]), int(frames[1])
        else:
            frames, fptr, n = _host_list(frames, FRAME_DTYPE)
        lptr = None
        if isinstance(levels, int):
            lptr = levels
        elif levels is not None:
            levels, lptr, _ = _host_list(levels, LEVEL_DTYPE, n)
        cfg = _wire_cfg(format, levels is not None, tick_bias, short)
        room = L.ADSB_WIRE_MAX_BYTES * n if cap is None else int(cap)
        out = np.zeros(max(room, 1), dtype=np.uint8)
        ends = np.zeros(max(n, 1), dtype=np.uint32)
        total = C.c_size_t()
        L.check(self._lib.adsb_wire_of(self._h, C.byref(cfg), fptr, lptr, n, out.ctypes.data, room, C.byref(total),
                                       ends.ctypes.data), "adsb_wire_of")
        return _wire_result(out, room, ends[:n].copy(), total.value)

    def wire_in_of_async(self, data, stream_ends=None, format="beast", filter=0, tick_bias=0, max_frames=0,
                         levels=False):
        """adsb_wire_in_of alone: enqueues the parse of one or many streams of Beast binary or AVR text and returns once
        the host arrays are copied.  data: bytes-like or a uint8 array (host), or (device pointer, length); stream_ends:
        the streams' ascending exclusive ends (None: one stream).  See host_wire_parse for the rest; the level records
        are on this context's sample type's full scale."""
        keep, ptr, n, ends = _wire_in_input(data, stream_ends)
        cfg = _wire_in_cfg(format, filter, tick_bias, max_frames, self.sample_type, levels)
        L.check(self._lib.adsb_wire_in_of(self._h, C.byref(cfg), ptr, n, ends.ctypes.data if len(ends) else None,
                                          len(ends)), "adsb_wire_in_of")
        self._wire_in = (len(ends), bool(levels))

    def fetch_wire_in(self):
        """adsb_fetch_wire_in: waits for the parse wire_in_of_async() enqueued -> WireIn."""
        n_streams, levels = getattr(self, "_wire_in", (0, False))
        hdr, got = L.AdsbWireInHeader(), C.c_size_t()
        L.check(self._lib.adsb_fetch_wire_in(self._h, None, None, None, 0, C.byref(got), None, None, 0, C.byref(hdr)),
                "adsb_fetch_wire_in")                 # the sizes first; the lists stay where they are
        room = int(hdr.n_frames)
        fr, rx = np.zeros(max(room, 1), dtype=FRAME_DTYPE), np.zeros(max(room, 1), dtype=WIRE_RX_DTYPE)
        lv = np.zeros(max(room, 1), dtype=LEVEL_DTYPE) if levels else None
        counts, consumed = np.zeros(n_streams, dtype=np.uint64), np.zeros(n_streams, dtype=np.uint64)
        L.check(self._lib.adsb_fetch_wire_in(self._h, fr.ctypes.data, rx.ctypes.data,
                                             None if lv is None else lv.ctypes.data, room, C.byref(got),
                                             counts.ctypes.data if n_streams else None,
                                             consumed.ctypes.data if n_streams else None, n_streams, C.byref(hdr)),
                "adsb_fetch_wire_in")
        return _wire_in_result(fr, rx, lv, got.value, counts, consumed, hdr)

    def wire_in_of(self, data, stream_ends=None, format="beast", filter=0, tick_bias=0, max_frames=0, levels=False):
        """Beast binary or AVR text back into frames, parsed on the device -> WireIn (frames, rx, levels, counts,
        consumed, header).  frames / levels / counts are arguments for correlate_of, TrackBank.update and wire_of;
        consumed[r] is where stream r's next chunk starts.  See wire_in_of_async."""
        self.wire_in_of_async(data, stream_ends, format, filter, tick_bias, max_frames, levels)
        return self.fetch_wire_in()

    def wire_in_device(self):
        """adsb_wire_in_device: device addresses (frames, rx, levels or None, counts, consumed, header); no
        synchronisation."""
        p = [C.c_void_p() for _ in range(6)]
        L.check(self._lib.adsb_wire_in_device(self._h, *[C.byref(x) for x in p]), "adsb_wire_in_device")
        return tuple(x.value for x in p)

    def modes_of_async(self, frames, counts=None, known=None):
        """adsb_modes_of alone: enqueues and returns once the host arrays are copied.  frames: a FRAME_DTYPE array (host)
        or (device pointer, count); counts: frames per receiver or None; known: None, an ascending unique uint32 array,
        a (device pointer, count) pair (modes_device()[1] with the last header's n_known_out) or a TrackTable."""
        if isinstance(frames, tuple):
            fptr, n = (int(frames[0]) if int(frames[1]) else None), int(frames[1])
        else:
            frames, fptr, n = _host_list(frames, FRAME_DTYPE)
        karr, kptr, nk = _known_list(known)
        cnt = None if counts is None else np.ascontiguousarray(counts, dtype=np.uint64).reshape(-1)
        L.check(self._lib.adsb_modes_of(self._h, fptr, n, None if cnt is None else cnt.ctypes.data,
                                        0 if cnt is None else len(cnt), kptr, nk), "adsb_modes_of")
        self._modes = 0 if cnt is None else len(cnt)

    def fetch_modes(self):
        """adsb_fetch_modes: waits for the last modes_of_async() -> (MODES_DTYPE records, uint32 known_out, FRAME_DTYPE
        squitters, uint64 squitter_counts or None, the MODES_HEADER_DTYPE record)."""
        R, hdr = getattr(self, "_modes", 0), L.AdsbModesHeader()
        L.check(self._lib.adsb_fetch_modes(self._h, None, 0, None, 0, None, 0, None, 0, C.byref(hdr)),
                "adsb_fetch_modes")                   # the sizes first; the lists stay where they are
        n, nk, ns = int(hdr.n), int(hdr.n_known_out), int(hdr.n_squitters)
        recs, kout = np.zeros(max(n, 1), dtype=MODES_DTYPE), np.zeros(max(nk, 1), dtype=np.uint32)
        sq, sqc = np.zeros(max(ns, 1), dtype=FRAME_DTYPE), np.zeros(max(R, 1), dtype=np.uint64)
        L.check(self._lib.adsb_fetch_modes(self._h, recs.ctypes.data, n, kout.ctypes.data, nk, sq.ctypes.data, ns,
                                           sqc.ctypes.data if R else None, R, C.byref(hdr)), "adsb_fetch_modes")
        header = np.frombuffer(bytes(hdr), dtype=MODES_HEADER_DTYPE)[0]
        return recs[:n].copy(), kout[:nk].copy(), sq[:ns].copy(), (sqc[:R].copy() if R else None), header

    def modes_of(self, frames, counts=None, known=None):
        """adsb_modes_of + adsb_fetch_modes: every frame's address, kind (MODES_KINDS) and Mode S surveillance fields ->
        (recs, known_out, squitters, squitter_counts, header).  known_out is the next call's `known`; squitters (the
        SELF DF17/18 frames) and squitter_counts are arguments for TrackTable.update / TrackBank.update.  See
        modes_of_async."""
        self.modes_of_async(frames, counts, known)
        return self.fetch_modes()

    def modes_device(self):
        """adsb_modes_device: device addresses (records, known_out, squitters, squitter_counts or None, header); no
        synchronisation."""
        p = [C.c_void_p() for _ in range(5)]
        L.check(self._lib.adsb_modes_device(self._h, *[C.byref(x) for x in p]), "adsb_modes_device")
        return tuple(x.value for x in p)

    def commb_of_async(self, frames):
        """adsb_commb_of alone: enqueues and returns once a host list is copied.  frames: a FRAME_DTYPE array (host) or
        (device pointer, count), for example wire_in_device()[0] with the parse's frame count."""
        if isinstance(frames, tuple):
            fptr, n = (int(frames[0]) if int(frames[1]) else None), int(frames[1])
        else:
            frames, fptr, n = _host_list(frames, FRAME_DTYPE)
        L.check(self._lib.adsb_commb_of(self._h, fptr, n), "adsb_commb_of")

    def fetch_commb(self):
        """adsb_fetch_commb: waits for the last commb_of_async() -> (COMMB_DTYPE records, the COMMB_HEADER_DTYPE
        record)."""
        hdr = L.AdsbCommbHeader()
        L.check(self._lib.adsb_fetch_commb(self._h, None, 0, C.byref(hdr)), "adsb_fetch_commb")   # the size first
        n = int(hdr.n)
        recs = np.zeros(max(n, 1), dtype=COMMB_DTYPE)
        L.check(self._lib.adsb_fetch_commb(self._h, recs.ctypes.data, n, C.byref(hdr)), "adsb_fetch_commb")
        return recs[:n].copy(), np.frombuffer(bytes(hdr), dtype=COMMB_HEADER_DTYPE)[0]

    def commb_of(self, frames):
        """adsb_commb_of + adsb_fetch_commb: for every DF20/21 frame the Comm-B register its MB field carries, inferred
        from the 56 bits (state: COMMB_STATES), and that register's values -> (recs, header), index for index with the
        list and with modes_of's records.  commb_physical(recs) gives the values in physical units.  See
        commb_of_async."""
        self.commb_of_async(frames)
        return self.fetch_commb()

    def commb_device(self):
        """adsb_commb_device: device addresses (records, header); no synchronisation."""
        p = [C.c_void_p() for _ in range(2)]
        L.check(self._lib.adsb_commb_device(self._h, *[C.byref(x) for x in p]), "adsb_commb_device")
        return tuple(x.value for x in p)

    def es_of_async(self, frames):
        """adsb_es_of alone: enqueues and returns once a host list is copied.  frames: a FRAME_DTYPE array (host) or
        (device pointer, count), for example modes_device()[2] with the squitter count."""
        if isinstance(frames, tuple):
            fptr, n = (int(frames[0]) if int(frames[1]) else None), int(frames[1])
        else:
            frames, fptr, n = _host_list(frames, FRAME_DTYPE)
        L.check(self._lib.adsb_es_of(self._h, fptr, n), "adsb_es_of")

    def fetch_es(self):
        """adsb_fetch_es: waits for the last es_of_async() -> (ES_DTYPE records, the ES_HEADER_DTYPE record)."""
        hdr = L.AdsbEsHeader()
        L.check(self._lib.adsb_fetch_es(self._h, None, 0, C.byref(hdr)), "adsb_fetch_es")   # the size first
        n = int(hdr.n)
        recs = np.zeros(max(n, 1), dtype=ES_DTYPE)
        L.check(self._lib.adsb_fetch_es(self._h, recs.ctypes.data, n, C.byref(hdr)), "adsb_fetch_es")
        return recs[:n].copy(), np.frombuffer(bytes(hdr), dtype=ES_HEADER_DTYPE)[0]

    def es_of(self, frames):
        """adsb_es_of + adsb_fetch_es: for every DF17/18 frame what it says about the aircraft's status (state:
        ES_STATES; the emitter category, the emergency state and squawk, the ACAS RA, the target state, the operational
        status, NACv and NIC supplement B) -> (recs, header), index for index with the list and with modes_of's
        records.  es_physical(recs) gives the values in physical units.  See es_of_async."""
        self.es_of_async(frames)
        return self.fetch_es()

    def es_device(self):
        """adsb_es_device: device addresses (records, header); no synchronisation."""
        p = [C.c_void_p() for _ in range(2)]
        L.check(self._lib.adsb_es_device(self._h, *[C.byref(x) for x in p]), "adsb_es_device")
        return tuple(x.value for x in p)

    def replies_of_async(self, iq, n_channels=1, n_samples=None, channel_stride=None, known=None, ap="all", max_frames=0,
                         first_sample=0):
        """adsb_replies_of alone: enqueues the replies scan and returns once a host known[] is copied.  iq: a device
        pointer (then n_samples is needed) or a device tensor of I,Q pairs (data_ptr() and numel()); known: None, an
        ascending unique uint32 array, a (device pointer, count) pair or a TrackTable; ap: "all" or "known"."""
        if hasattr(iq, "data_ptr"):
            if n_samples is None:
                n_samples = int(iq.numel()) // 2 // int(n_channels)
            iq = iq.data_ptr()
        if n_samples is None:
            raise ValueError("n_samples is needed with a device pointer")
        stride = int(n_samples) if channel_stride is None else int(channel_stride)
        karr, kptr, nk = _known_list(known)
        cfg = _replies_cfg(ap, max_frames, first_sample)
        L.check(self._lib.adsb_replies_of(self._h, C.byref(cfg), int(iq), int(n_channels), int(n_samples), stride, kptr, nk),
                "adsb_replies_of")
        self._replies_channels = int(n_channels)

    def fetch_replies(self):
        """adsb_fetch_replies: waits for the last replies_of_async() -> (FRAME_DTYPE frames, uint64 counts per channel,
        the REPLIES_HEADER_DTYPE record)."""
        nch, hdr = getattr(self, "_replies_channels", 1), L.AdsbRepliesHeader()
        L.check(self._lib.adsb_fetch_replies(self._h, None, 0, None, None, C.byref(hdr)), "adsb_fetch_replies")  # the size first
        n = int(hdr.n_out)
        out, counts, got = np.zeros(max(n, 1), dtype=FRAME_DTYPE), np.zeros(max(nch, 1), dtype=np.uint64), C.c_size_t()
        L.check(self._lib.adsb_fetch_replies(self._h, out.ctypes.data, n, C.byref(got), counts.ctypes.data, C.byref(hdr)),
                "adsb_fetch_replies")
        return out[:got.value].copy(), counts[:nch].copy(), np.frombuffer(bytes(hdr), dtype=REPLIES_HEADER_DTYPE)[0]

    def replies_of(self, iq, n_channels=1, n_samples=None, channel_stride=None, known=None, ap="all", max_frames=0,
                   first_sample=0):
        """adsb_replies_of + adsb_fetch_replies: the Mode S replies (DF11, DF18 and the address/parity formats DF0, 4, 5,
        16, 20, 21) in a sample buffer on the device, by the scan of include/adsb_hip.h "Mode S replies from samples" ->
        (frames, counts, header).  The list drops into modes_of, commb_of and correlate_of; merge_lists puts it and the
        demodulator's list into one.  See replies_of_async."""
        self.replies_of_async(iq, n_channels, n_samples, channel_stride, known, ap, max_frames, first_sample)
        return self.fetch_replies()

    def replies_device(self):
        """adsb_replies_device: device addresses (frames, counts, header); no synchronisation."""
        p = [C.c_void_p() for _ in range(3)]
        L.check(self._lib.adsb_replies_device(self._h, *[C.byref(x) for x in p]), "adsb_replies_device")
        return tuple(x.value for x in p)

    def merge_lists(self, a, counts_a, b, counts_b):
        """adsb_merge_lists_of: two lists in fetch's layout as one, on the device -> (frames, src, counts); see
        host_merge_lists.  a, b: FRAME_DTYPE arrays (host) or (device pointer, count) pairs; counts_a, counts_b: frames
        per channel (host)."""
        ca, cb = (np.ascontiguousarray(x, dtype=np.uint64).reshape(-1) for x in (counts_a, counts_b))
        if len(ca) != len(cb):
            raise ValueError("counts_a and counts_b differ in length")
        ptr = []
        for lst, cnt in ((a, ca), (b, cb)):
            if isinstance(lst, tuple):
                arr, p, n = None, (int(lst[0]) if int(lst[1]) else None), int(lst[1])
            else:
                arr, p, n = _host_list(lst, FRAME_DTYPE)
            if n != int(cnt.sum()):
                raise ValueError("counts do not describe the lists")
            ptr.append((arr, p, n))
        n = ptr[0][2] + ptr[1][2]
        out, src = np.zeros(max(n, 1), dtype=FRAME_DTYPE), np.zeros(max(n, 1), dtype=np.uint32)
        counts = np.zeros(max(len(ca), 1), dtype=np.uint64)
        L.check(self._lib.adsb_merge_lists_of(self._h, ptr[0][1], ca.ctypes.data, ptr[1][1], cb.ctypes.data, len(ca),
                                              out.ctypes.data, src.ctypes.data, counts.ctypes.data), "adsb_merge_lists_of")
        return out[:n].copy(), src[:n].copy(), counts[:len(ca)].copy()

    host_replies = staticmethod(host_replies)
    host_merge_lists = staticmethod(host_merge_lists)

    def correlate_async(self, window, sample_base=None, levels=False):
        """adsb_correlate_launch alone: the last launch's list, channel k as receiver k, correlated on the device.
        window: samples; sample_base: one uint64 per channel (None: zeros); levels: take the launch's levels (enqueued
        here if they have not been) for best_receiver / best_signal_sum."""
        base, bptr = _u64_list(sample_base, self._last_channels, "sample_base")
        cfg = L.AdsbCorrelateCfg(int(window), 1 if levels else 0, 0)
        L.check(self._lib.adsb_correlate_launch(self._h, C.byref(cfg), bptr), "adsb_correlate_launch")

    def correlate(self, window, sample_base=None, levels=False):
        """The last launch's frames as one de-duplicated, time-ordered message list: (messages, frames, receptions) as
        MESSAGE_DTYPE, FRAME_DTYPE and RECEPTION_DTYPE arrays.  See correlate_async."""
        self.correlate_async(window, sample_base, levels)
        return self.fetch_correlated()

    def correlate_of(self, frames, counts, window, sample_base=None, levels=None):
        """adsb_correlate_of: any multi-receiver list -> (messages, frames, receptions).  frames: a FRAME_DTYPE array
        (host) or (device pointer, count), receiver 0's frames first, counts[r] each; levels: None, a LEVEL_DTYPE array
        (host) or a device pointer; sample_base: one uint64 per receiver (None: zeros); window: samples."""
        self.correlate_of_async(frames, counts, window, sample_base, levels)
        return self.fetch_correlated()

    def correlate_of_async(self, frames, counts, window, sample_base=None, levels=None):
        """adsb_correlate_of alone: enqueues and returns once the host arrays are copied."""
        if isinstance(frames, tuple):
            fptr, n = int(frames[0]), int(frames[1])
        else:
            frames, fptr, n = _host_list(frames, FRAME_DTYPE)
        lptr = None
        if isinstance(levels, int):
            lptr = levels
        elif levels is not None:
            levels, lptr, _ = _host_list(levels, LEVEL_DTYPE, n)
        counts = np.ascontiguousarray(counts, dtype=np.uint64).reshape(-1)
        base, bptr = _u64_list(sample_base, len(counts), "sample_base")
        cfg = L.AdsbCorrelateCfg(int(window), 0, 0)
        L.check(self._lib.adsb_correlate_of(self._h, C.byref(cfg), fptr, lptr, n,
                                            counts.ctypes.data if len(counts) else None, len(counts), bptr),
                "adsb_correlate_of")

    def fetch_correlated(self):
        """adsb_fetch_correlated: waits for the last correlate call -> (messages, frames, receptions); frames are the
        messages' first 24 bytes, the list correlated_device() has on the device."""
        n_msgs, n_recs = C.c_size_t(), C.c_size_t()
        L.check(self._lib.adsb_fetch_correlated(self._h, None, 0, C.byref(n_msgs), None, 0, C.byref(n_recs)),
                "adsb_fetch_correlated")
        msgs = np.zeros(max(n_msgs.value, 1), dtype=MESSAGE_DTYPE)
        recs = np.zeros(max(n_recs.value, 1), dtype=RECEPTION_DTYPE)
        L.check(self._lib.adsb_fetch_correlated(self._h, msgs.ctypes.data, n_msgs.value, C.byref(n_msgs), recs.ctypes.data,
                                                n_recs.value, C.byref(n_recs)), "adsb_fetch_correlated")
        msgs = msgs[:n_msgs.value].copy()
        return msgs, frames_of_messages(msgs), recs[:n_recs.value].copy()

    def correlated_counts(self):
        """(messages, receptions) of the last correlate call: waits for it and reads the two counts, nothing else; the
        lists stay where they are (correlated_device())."""
        n_msgs, n_recs = C.c_size_t(), C.c_size_t()
        L.check(self._lib.adsb_fetch_correlated(self._h, None, 0, C.byref(n_msgs), None, 0, C.byref(n_recs)),
                "adsb_fetch_correlated")
        return n_msgs.value, n_recs.value

    def correlated_device(self):
        """adsb_correlated_device: device addresses (messages, frames, receptions, {u64 n_messages, u64 n_receptions});
        no synchronisation."""
        m, f, r, h = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        L.check(self._lib.adsb_correlated_device(self._h, C.byref(m), C.byref(f), C.byref(r), C.byref(h)),
                "adsb_correlated_device")
        return m.value, f.value, r.value, h.value

    def multilaterate_async(self, receivers, rx=None, **cfg):
        """adsb_multilaterate alone: the last correlate call's result, solved where it lies on the device; nothing is
        read back.  rx: None, a WIRE_RX_DTYPE array (host) or a device pointer (wire_in_device()[1]) with one record per
        frame of the correlated list.  See host_multilaterate for receivers and the keywords."""
        rcv = _mlat_receivers(receivers)
        c = _mlat_cfg(**cfg)
        keep, xptr = (None, rx) if isinstance(rx, int) else _mlat_list(rx, WIRE_RX_DTYPE)[:2]
        L.check(self._lib.adsb_multilaterate(self._h, C.byref(c), rcv.ctypes.data if len(rcv) else None, len(rcv), xptr),
                "adsb_multilaterate")

    def multilaterate(self, receivers, rx=None, clocks=False, clock_cfg=None, **cfg):
        """Where each message of the last correlate call was sent from -> (MLAT_FIX_DTYPE fixes, header).  See
        multilaterate_async.  clocks=True: clock sync first (clock_cfg: clock_sync's keywords beyond the times, which
        are cfg's), then the corrected receptions, then the solver on those, in stream order with ONE host wait: the
        solver's entry point takes the lists' lengths from the host, so the two counts of the correlate header are read
        after sync and apply have been enqueued.  The receivers' clock_offset_s are then the sync's priors."""
        if not clocks:
            self.multilaterate_async(receivers, rx, **cfg)
            return self.fetch_mlat()
        self.multilaterate_clocks_async(receivers, rx, clock_cfg, **cfg)
        return self.fetch_mlat()

    def multilaterate_clocks_async(self, receivers, rx=None, clock_cfg=None, **cfg):
        """multilaterate(clocks=True) without the fetch: everything stays on the device (mlat_device(),
        correlated_device()); only the two list lengths are read back -> (messages, receptions) of the correlate
        result, e.g. for TrackTable.update_device(frames_dev, messages, mlat_ptr=fixes_dev)."""
        times = {k: cfg[k] for k in ("time_source", "seconds_per_tick") if k in cfg}
        self.clock_sync_async(receivers, rx, **dict(times, **(clock_cfg or {})))
        self.clock_apply_async()
        spt = float(cfg.get("seconds_per_tick") or 1.0 / 12e6)
        plain = _mlat_receivers(receivers).copy()
        plain["clock_offset_s"] = 0.0
        msgs_dev, _, _, hdr_dev = self.correlated_device()
        recs_dev, n = self.clock_receptions_device()
        # the lists where they lie; the solver's entry point takes their lengths from the host, so the two counts of the
        # correlate header are read here, behind everything enqueued above
        n_msgs, n_recs = C.c_size_t(), C.c_size_t()
        L.check(self._lib.adsb_fetch_correlated(self._h, None, 0, C.byref(n_msgs), None, 0, C.byref(n_recs)),
                "adsb_fetch_correlated")
        rest = {k: v for k, v in cfg.items() if k not in ("time_source", "seconds_per_tick")}
        self.multilaterate_of_async(plain, (msgs_dev, n_msgs.value), (recs_dev, min(n, n_recs.value)), None,
                                    time_source="reception", seconds_per_tick=spt / 256.0, **rest)
        return n_msgs.value, n_recs.value

    def clock_sync_async(self, receivers, rx=None, **cfg):
        """adsb_clock_sync alone: the last correlate call's result, where it lies on the device.  rx as for
        multilaterate_async.  See host_clock_sync for receivers and the keywords."""
        rcv = _mlat_receivers(receivers)
        c = _clock_cfg(**cfg)
        keep, xptr = (None, rx) if isinstance(rx, int) else _mlat_list(rx, WIRE_RX_DTYPE)[:2]
        L.check(self._lib.adsb_clock_sync(self._h, C.byref(c), rcv.ctypes.data if len(rcv) else None, len(rcv), xptr),
                "adsb_clock_sync")

    def clock_sync(self, receivers, rx=None, **cfg):
        """Every receiver's clock against the reference, from the position messages of the last correlate call ->
        (CLOCK_DTYPE clocks, the CLOCK_HEADER_DTYPE record).  clock_apply() then corrects the receptions."""
        self.clock_sync_async(receivers, rx, **cfg)
        return self.fetch_clocks()

    def clock_sync_of_async(self, receivers, messages, receptions, rx=None, **cfg):
        """adsb_clock_sync_of alone: any correlate result, each list a host array or a (device pointer, count) pair."""
        rcv = _mlat_receivers(receivers)
        c = _clock_cfg(**cfg)
        msgs, mptr, nm = _mlat_list(messages, MESSAGE_DTYPE)
        recs, rptr, nr = _mlat_list(receptions, RECEPTION_DTYPE)
        rxa, xptr, nx = _mlat_list(rx, WIRE_RX_DTYPE)
        L.check(self._lib.adsb_clock_sync_of(self._h, C.byref(c), rcv.ctypes.data if len(rcv) else None, len(rcv), mptr,
                                             nm, rptr, nr, xptr, nx), "adsb_clock_sync_of")

    def clock_sync_of(self, receivers, messages, receptions, rx=None, **cfg):
        """adsb_clock_sync_of -> (clocks, header).  See host_clock_sync, its CPU mirror."""
        self.clock_sync_of_async(receivers, messages, receptions, rx, **cfg)
        return self.fetch_clocks()

    def fetch_clocks(self):
        """adsb_fetch_clocks: waits for the last clock-sync call -> (clocks, the CLOCK_HEADER_DTYPE record)."""
        hdr, got = L.AdsbClockHeader(), C.c_size_t()
        clocks = np.zeros(256, dtype=CLOCK_DTYPE)
        rc = self._lib.adsb_fetch_clocks(self._h, clocks.ctypes.data, 256, C.byref(got), C.byref(hdr))
        if rc != L.ADSB_OK and not (rc == L.ADSB_E_ARG and hdr.flags & L.ADSB_CLOCK_HDR_BAD_INDEX):
            L.check(rc, "adsb_fetch_clocks")
        return clocks[:got.value].copy(), np.frombuffer(bytes(hdr), dtype=CLOCK_HEADER_DTYPE)[0]

    def clocks_device(self):
        """adsb_clocks_device: device addresses (clocks, header); no synchronisation."""
        k, h = C.c_void_p(), C.c_void_p()
        L.check(self._lib.adsb_clocks_device(self._h, C.byref(k), C.byref(h)), "adsb_clocks_device")
        return k.value, h.value

    def clock_apply_async(self):
        """adsb_clock_apply alone: the last clock sync's receptions with corrected times, on the device."""
        L.check(self._lib.adsb_clock_apply(self._h), "adsb_clock_apply")

    def clock_apply(self):
        """adsb_clock_apply -> the corrected RECEPTION_DTYPE list, times in units of seconds_per_tick / 256: an argument
        for multilaterate_of(..., time_source="reception", seconds_per_tick=spt / 256) with all clock offsets 0."""
        self.clock_apply_async()
        got, total = C.c_size_t(), C.c_size_t()
        L.check(self._lib.adsb_fetch_clock_receptions(self._h, None, 0, C.byref(got), C.byref(total)),
                "adsb_fetch_clock_receptions")
        out = np.zeros(max(total.value, 1), dtype=RECEPTION_DTYPE)
        L.check(self._lib.adsb_fetch_clock_receptions(self._h, out.ctypes.data, total.value, C.byref(got), C.byref(total)),
                "adsb_fetch_clock_receptions")
        return out[:got.value].copy()

    def clock_receptions_device(self):
        """adsb_clock_receptions_device: (device address of the corrected receptions, their count's upper bound)."""
        p, n = C.c_void_p(), C.c_size_t()
        L.check(self._lib.adsb_clock_receptions_device(self._h, C.byref(p), C.byref(n)), "adsb_clock_receptions_device")
        return p.value, n.value

    def multilaterate_of_async(self, receivers, messages, receptions, rx=None, **cfg):
        """adsb_multilaterate_of alone: any correlate result, each list a host array or a (device pointer, count)
        pair; enqueues and returns once the host arrays are copied."""
        rcv = _mlat_receivers(receivers)
        c = _mlat_cfg(**cfg)
        msgs, mptr, nm = _mlat_list(messages, MESSAGE_DTYPE)
        recs, rptr, nr = _mlat_list(receptions, RECEPTION_DTYPE)
        rxa, xptr, nx = _mlat_list(rx, WIRE_RX_DTYPE)
        L.check(self._lib.adsb_multilaterate_of(self._h, C.byref(c), rcv.ctypes.data if len(rcv) else None, len(rcv), mptr,
                                                nm, rptr, nr, xptr, nx), "adsb_multilaterate_of")

    def multilaterate_of(self, receivers, messages, receptions, rx=None, **cfg):
        """adsb_multilaterate_of -> (MLAT_FIX_DTYPE fixes, header).  See host_multilaterate, its CPU mirror."""
        self.multilaterate_of_async(receivers, messages, receptions, rx, **cfg)
        return self.fetch_mlat()

    def fetch_mlat(self):
        """adsb_fetch_mlat: waits for the last multilaterate call -> (fixes, the MLAT_HEADER_DTYPE record)."""
        hdr, got = L.AdsbMlatHeader(), C.c_size_t()
        rc = self._lib.adsb_fetch_mlat(self._h, None, 0, C.byref(got), C.byref(hdr))   # the count first
        if rc not in (L.ADSB_OK, L.ADSB_E_ARG):
            L.check(rc, "adsb_fetch_mlat")
        n = int(hdr.n_messages)
        fixes = np.zeros(max(n, 1), dtype=MLAT_FIX_DTYPE)
        L.check(self._lib.adsb_fetch_mlat(self._h, fixes.ctypes.data, n, C.byref(got), C.byref(hdr)), "adsb_fetch_mlat")
        return fixes[:got.value].copy(), np.frombuffer(bytes(hdr), dtype=MLAT_HEADER_DTYPE)[0]

    def mlat_device(self):
        """adsb_mlat_device: device addresses (fixes, header); no synchronisation."""
        f, h = C.c_void_p(), C.c_void_p()
        L.check(self._lib.adsb_mlat_device(self._h, C.byref(f), C.byref(h)), "adsb_mlat_device")
        return f.value, h.value

    def set_result_target(self, dev_ptr, nbytes):
        """Next launches write [32-byte header | frames] straight into caller-owned HBM (None: reset)."""
        L.check(self._lib.adsb_set_result_target(self._h, dev_ptr, nbytes), "adsb_set_result_target")

    def set_stream_base(self, first_sample_index):
        """Frames of the following launches carry offset = first_sample_index + index inside the buffer."""
        L.check(self._lib.adsb_set_stream_base(self._h, int(first_sample_index)), "adsb_set_stream_base")

    def stream_wait_results(self, stream):
        """Make `stream` (hipStream_t as int) wait for the last launch's ordered frame list."""
        L.check(self._lib.adsb_stream_wait_results(self._h, stream), "adsb_stream_wait_results")

    # -- measurement / test helpers -------------------------------------------------------------------
    def timing_enable(self, every=1):
        """every = N > 0: attach timing events to every N-th launch; 0/False: off."""
        L.check(self._lib.adsb_timing_enable(self._h, int(every)), "adsb_timing_enable")

    def timing_read(self):
        a, b, n = C.c_double(), C.c_double(), C.c_uint32()
        L.check(self._lib.adsb_timing_read(self._h, C.byref(a), C.byref(b), C.byref(n)),
                "adsb_timing_read")
        return a.value, b.value, n.value

    def timing_read3(self):
        """(scan_ms, decode_ms, order_ms, n_launches): the three kernels of a launch, mean per timed launch."""
        a, b, c, n = C.c_double(), C.c_double(), C.c_double(), C.c_uint32()
        L.check(self._lib.adsb_timing_read3(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(n)), "adsb_timing_read3")
        return a.value, b.value, c.value, n.value

    def time_read_ceiling(self, dev_ptr, nbytes, iters=10):
        ms = C.c_double()
        L.check(self._lib.adsb_time_read_ceiling(self._h, dev_ptr, nbytes, iters, C.byref(ms)),
                "adsb_time_read_ceiling")
        return ms.value

    def magnitudes(self, iq):
        iq = np.ascontiguousarray(iq, dtype=self._np_dtype)
        n = iq.shape[0]
        out = np.empty(n, dtype=np.uint16)
        L.check(self._lib.adsb_debug_magnitudes(self._h, iq.ctypes.data, n, out.ctypes.data),
                "adsb_debug_magnitudes")
        return out

    def nsq_values(self, iq):
        """I^2 + Q^2 + 72 per i8 sample through the scan kernel's packing code (0xFFFF: the two paths disagree)."""
        iq = np.ascontiguousarray(iq, dtype=np.int8)
        n = iq.shape[0]
        out = np.empty(n, dtype=np.uint16)
        L.check(self._lib.adsb_debug_nsq_values(self._h, iq.ctypes.data, n, out.ctypes.data), "adsb_debug_nsq_values")
        return out

    def synth_fill_device(self, cfg, channel, first_sample, n_samples, dev_ptr):
        L.check(self._lib.adsb_synth_fill_device(self._h, C.byref(cfg), channel, first_sample,
                                                 n_samples, dev_ptr), "adsb_synth_fill_device")

    # -- reference thread structure (playback + stream mode) ------------------------------------------
    def pipeline_playback(self, data, chunk_len=20000, max_frames=1 << 20, want_text=True):
        data = np.ascontiguousarray(data, dtype=self._np_dtype)
        n = data.shape[0]
        frames = np.zeros(max_frames, dtype=FRAME_DTYPE)
        n_frames, n_buf, text_len = C.c_size_t(), C.c_uint64(), C.c_size_t()
        cap = 1 << 26 if want_text else 0
        text = C.create_string_buffer(cap) if want_text else None
        L.check(self._lib.adsb_pipeline_playback(self._h, self.sample_type, data.ctypes.data, n,
                                                 chunk_len,
                                                 frames.ctypes.data_as(C.POINTER(L.AdsbFrame)),
                                                 max_frames, C.byref(n_frames), C.byref(n_buf), text,
                                                 cap, C.byref(text_len)), "adsb_pipeline_playback")
        txt = text.value.decode() if want_text else None
        return frames[:min(n_frames.value, max_frames)].copy(), n_buf.value, txt

    def pipeline_run(self, data, chunk_len=20000, carry=False, send_tail=False, max_frames=1 << 20, want_text=True):
        """adsb_pipeline_run: playback thread -> GPU thread 2 (streaming front end) -> stream-mode text."""
        data = np.ascontiguousarray(data, dtype=self._np_dtype)
        frames = np.zeros(max_frames, dtype=FRAME_DTYPE)
        n_frames, n_buf, text_len = C.c_size_t(), C.c_uint64(), C.c_size_t()
        cap = 1 << 26 if want_text else 0
        text = C.create_string_buffer(cap) if want_text else None
        flags = (L.ADSB_REPLAY_CARRY if carry else 0) | (L.ADSB_REPLAY_SEND_TAIL if send_tail else 0)
        L.check(self._lib.adsb_pipeline_run(self._h, self.sample_type, data.ctypes.data, data.shape[0], chunk_len, flags,
                                            frames.ctypes.data_as(C.POINTER(L.AdsbFrame)), max_frames, C.byref(n_frames),
                                            C.byref(n_buf), text, cap, C.byref(text_len)), "adsb_pipeline_run")
        return frames[:min(n_frames.value, max_frames)].copy(), n_buf.value, (text.value.decode() if want_text else None)

    def replay_file(self, path, file_format=None, chunk_len=20000, carry=False, send_tail=False, max_frames=1 << 20):
        """adsb_replay_file: `.c16` (ctx i16) or raw rtl_sdr u8 (ctx i8) file -> (frames, n_buffers, n_samples, text)."""
        if file_format is None:
            file_format = L.ADSB_FILE_C16 if self.sample_type == L.ADSB_SAMPLE_I16 else L.ADSB_FILE_U8
        frames = np.zeros(max_frames, dtype=FRAME_DTYPE)
        n_frames, n_buf, n_samp, text_len = C.c_size_t(), C.c_uint64(), C.c_uint64(), C.c_size_t()
        cap = 1 << 26
        text = C.create_string_buffer(cap)
        flags = (L.ADSB_REPLAY_CARRY if carry else 0) | (L.ADSB_REPLAY_SEND_TAIL if send_tail else 0)
        L.check(self._lib.adsb_replay_file(self._h, os.fsencode(path), file_format, chunk_len, flags,
                                           frames.ctypes.data_as(C.POINTER(L.AdsbFrame)), max_frames, C.byref(n_frames),
                                           C.byref(n_buf), C.byref(n_samp), text, cap, C.byref(text_len)),
                "adsb_replay_file")
        return frames[:min(n_frames.value, max_frames)].copy(), n_buf.value, n_samp.value, text.value.decode()

    def pipeline_playback_carry(self, data, chunk_len=20000, max_frames=1 << 20):
        """Like pipeline_playback but thread 2 carries the last 240 samples over (not reference behaviour)."""
        data = np.ascontiguousarray(data, dtype=self._np_dtype)
        frames = np.zeros(max_frames, dtype=FRAME_DTYPE)
        n_frames, n_buf = C.c_size_t(), C.c_uint64()
        L.check(self._lib.adsb_pipeline_playback_carry(self._h, self.sample_type, data.ctypes.data, data.shape[0],
                                                       chunk_len, frames.ctypes.data_as(C.POINTER(L.AdsbFrame)),
                                                       max_frames, C.byref(n_frames), C.byref(n_buf)),
                "adsb_pipeline_playback_carry")
        return frames[:min(n_frames.value, max_frames)].copy(), n_buf.value


def group_plan(n_samples, n_members):
    """adsb_group_plan: [(first_sample, n_samples, n_offsets)] per member."""
    sh = (L.AdsbGroupShard * n_members)()
    L.check(L.load().adsb_group_plan(int(n_samples), int(n_members), sh), "adsb_group_plan")
    return [(s.first_sample, s.n_samples, s.n_offsets) for s in sh]


class AdsbGroup:
    """adsb_group_*: one buffer time-sharded over several contexts / devices behind one call (native: no torch,
    no launcher).  `devices` may repeat an ordinal (several contexts on one GPU)."""

    def __init__(self, devices, sample_type=L.ADSB_SAMPLE_I8, max_samples=1 << 20, max_out=1 << 16, root=0,
                 host_staging=True):
        self._lib = L.load()
        self._devs = (C.c_int32 * len(devices))(*devices)
        cfg = L.AdsbGroupCfg(L.ADSB_ABI_VERSION, sample_type, len(devices), root, self._devs, max_samples, max_out,
                             1 if host_staging else 0, 0)
        h = C.c_void_p()
        L.check(self._lib.adsb_group_create(C.byref(cfg), C.byref(h)), "adsb_group_create")
        self._h, self.n, self.max_out, self.sample_type = h, len(devices), max_out, sample_type
        self._np_dtype = np.int8 if sample_type == L.ADSB_SAMPLE_I8 else np.int16

    def close(self):
        if getattr(self, "_h", None):
            self._lib.adsb_group_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def demod(self, iq, max_out=None):
        """One host buffer through all members: (frames, flags)."""
        iq = np.ascontiguousarray(iq, dtype=self._np_dtype)
        n = iq.shape[0] if iq.ndim == 2 else iq.size // 2
        cap = self.max_out if max_out is None else max_out
        out = np.zeros(max(cap, 1), dtype=FRAME_DTYPE)
        n_out, flags = C.c_size_t(), C.c_uint32()
        L.check(self._lib.adsb_group_demod(self._h, iq.ctypes.data, n, out.ctypes.data_as(C.POINTER(L.AdsbFrame)), cap,
                                           C.byref(n_out), C.byref(flags)), "adsb_group_demod")
        return out[:n_out.value].copy(), flags.value

    def demod_device_async(self, dev_ptrs, n_samples):
        arr = (C.c_void_p * self.n)(*[int(p) if p else None for p in dev_ptrs])
        L.check(self._lib.adsb_group_demod_device_async(self._h, arr, int(n_samples)), "adsb_group_demod_device_async")

    def fetch(self, max_out=None):
        cap = self.max_out if max_out is None else max_out
        out = np.zeros(max(cap, 1), dtype=FRAME_DTYPE)
        n_out, total, flags = C.c_size_t(), C.c_uint64(), C.c_uint32()
        L.check(self._lib.adsb_group_fetch(self._h, out.ctypes.data_as(C.POINTER(L.AdsbFrame)), cap, C.byref(n_out),
                                           C.byref(total), C.byref(flags)), "adsb_group_fetch")
        return out[:n_out.value].copy(), total.value, flags.value

    def result_device(self):
        """(blob device pointer, hipStream_t the merge was enqueued on)."""
        blob, stream = C.c_void_p(), C.c_void_p()
        L.check(self._lib.adsb_group_result_device(self._h, C.byref(blob), C.byref(stream)), "adsb_group_result_device")
        return blob.value, stream.value


class Feed:
    """Streaming front end (adsb_feed_*): push host buffers, pop their frames in order; two may be in flight."""

    def __init__(self, dem, max_chunk, carry=False, ring_slots=3):
        self._lib, self._dem = dem._lib, dem
        cfg = L.AdsbFeedCfg(int(max_chunk), 1 if carry else 0, int(ring_slots))
        h = C.c_void_p()
        L.check(self._lib.adsb_feed_open(dem.handle, C.byref(cfg), C.byref(h)), "adsb_feed_open")
        self._h, self.max_chunk, self.carry = h, int(max_chunk), bool(carry)

    def close(self):
        if self._h:
            self._lib.adsb_feed_close(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    @property
    def in_flight(self):
        return self._lib.adsb_feed_in_flight(self._h)

    @property
    def ready(self):
        """True when pop() would not wait for the GPU."""
        r = self._lib.adsb_feed_ready(self._h)
        if r < 0 or r > 1:
            raise L.AdsbError(r, "adsb_feed_ready")
        return bool(r)

    def push(self, iq):
        iq = np.ascontiguousarray(iq, dtype=self._dem._np_dtype)
        n = iq.shape[0] if iq.ndim == 2 else iq.size // 2
        L.check(self._lib.adsb_feed_push(self._h, iq.ctypes.data, n), "adsb_feed_push")

    def acquire(self):
        """A pinned ring slot as a numpy array of shape (max_chunk, 2) to fill in place; then push_acquired(n)."""
        p = C.c_void_p()
        L.check(self._lib.adsb_feed_acquire(self._h, C.byref(p)), "adsb_feed_acquire")
        itemsize = np.dtype(self._dem._np_dtype).itemsize
        buf = (C.c_char * (self.max_chunk * 2 * itemsize)).from_address(p.value)
        return np.frombuffer(buf, dtype=self._dem._np_dtype).reshape(self.max_chunk, 2)

    def push_acquired(self, n):
        L.check(self._lib.adsb_feed_push(self._h, None, int(n)), "adsb_feed_push")

    def pop(self, max_out=None):
        cap = self._dem.max_out if max_out is None else max_out
        out = np.zeros(max(cap, 1), dtype=FRAME_DTYPE)
        n_out, flags, first = C.c_size_t(), C.c_uint32(), C.c_uint64()
        ptr = out.ctypes.data_as(C.POINTER(L.AdsbFrame)) if cap else None    # (max_out = 0: no buffer at all)
        L.check(self._lib.adsb_feed_pop(self._h, ptr, cap, C.byref(n_out), C.byref(flags), C.byref(first)), "adsb_feed_pop")
        return out[:n_out.value].copy(), flags.value, first.value


class _TrackStore:
    """What TrackTable and TrackBank share: lifecycle, points, the summaries, and the helpers of the fetches.  A subclass
    sets _prefix, which selects its C functions (adsb_track_table_ / adsb_track_bank_)."""
    _prefix = None

    def _open(self, dem, cfg, max_frames):
        self._lib, self._dem = dem._lib, dem
        h = C.c_void_p()
        L.check(getattr(self._lib, self._prefix + "create")(dem.handle, C.byref(cfg), C.byref(h)), self._prefix + "create")
        self._h, self.max_frames = h, int(max_frames)

    def _call(self, name, *args):
        L.check(getattr(self._lib, self._prefix + name)(self._h, *args), self._prefix + name)

    def _fetch(self, name, dtypes, probe=(), extra=(), size=None):
        """<prefix><name>(handle, one buffer per dtype, max, &n, *extra): asks for n with no buffer (and `probe` in
        place of `extra`) unless the caller knows `size`, allocates, fetches; -> one array per dtype, n long."""
        n = C.c_size_t()
        if size is None:
            self._call(name, *[None] * len(dtypes), 0, C.byref(n), *probe)
            size = n.value
        outs = [np.zeros(max(size, 1), dtype=d) for d in dtypes]
        types = getattr(self._lib, self._prefix + name).argtypes[1:1 + len(dtypes)]
        self._call(name, *[o.ctypes.data_as(t) for o, t in zip(outs, types)], len(outs[0]), C.byref(n), *extra)
        return [o[:n.value].copy() for o in outs]

    def close(self):
        if getattr(self, "_h", None):
            getattr(self._lib, self._prefix + "destroy")(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        self._call("reset")

    def points(self):
        """One TRACK_POINT_DTYPE record per frame of the last update, in its list order."""
        return self._fetch("fetch_points", [TRACK_POINT_DTYPE], size=self.max_frames)[0]

    def summaries_reserve(self):
        """adsb_track_{table,bank}_summaries_reserve: from now on every update also leaves one summary per frame and
        the changed list on the device."""
        self._call("summaries_reserve")

    def summaries(self):
        """One AIRCRAFT_DTYPE record per frame of the last update, in its list order (a bank: receiver 0's frames
        first): the frame's aircraft (a bank: on its receiver) as it stands right after that frame, which is what the
        reference's web thread broadcasts per packet."""
        return self._fetch("fetch_summaries", [AIRCRAFT_DTYPE])[0]

    def summaries_device(self):
        """Device address of the last update's summaries; valid on the ctx stream, no synchronisation."""
        dev = C.c_void_p()
        self._call("summaries_device", C.byref(dev))
        return dev.value

    def levels_reserve(self):
        """adsb_track_{table,bank}_levels_reserve: one AIRCRAFT_LEVEL_DTYPE record beside every aircraft record, which
        an update given `levels` merges the frames' LEVEL_DTYPE records into."""
        self._call("levels_reserve")

    def levels_device(self):
        """Device address of the level records, one per record place in slot order (a bank: receiver r's from place
        r x max_aircraft); no synchronisation."""
        dev = C.c_void_p()
        self._call("levels_device", C.byref(dev))
        return dev.value

    def _fixes_reserve(self, sites, n):
        s = _sites(sites, n)
        self._call("fixes_reserve", s.ctypes.data_as(C.POINTER(L.AdsbSite)))

    def fixes_device(self):
        """Device address of the fixes, one per record place in slot order (as levels_device); no synchronisation."""
        dev = C.c_void_p()
        self._call("fixes_device", C.byref(dev))
        return dev.value

    def frame_fixes(self):
        """One FRAME_FIX_DTYPE record per frame of the last update, in its list order: the frame's own position from its
        receiver's site, ADSB_FIX_REJECTED if it was turned away, flags 0 if it is no position message."""
        return self._fetch("fetch_frame_fixes", [FRAME_FIX_DTYPE], size=self.max_frames)[0]

    @staticmethod
    def _host_levels(levels, n):
        """A host LEVEL_DTYPE array of n records -> (the array to keep alive, its address or None)."""
        levels = np.ascontiguousarray(levels, dtype=LEVEL_DTYPE)
        if len(levels) != n:
            raise ValueError(f"levels: {len(levels)} records for {n} frames")
        return levels, (levels.ctypes.data if n else None)


class TrackTable(_TrackStore):
    """adsb_track_table_*: one aircraft table on the device that lives across launches (the reference's
    HashMap<u32, Aircraft> of its display thread), fed one ordered frame list per update."""
    _prefix = "adsb_track_table_"

    def __init__(self, dem, max_aircraft=0, max_frames=1 << 16, seconds_per_sample=0.5e-6):
        self._open(dem, L.AdsbTrackTableCfg(L.ADSB_ABI_VERSION, int(max_aircraft), int(max_frames),
                                            float(seconds_per_sample)), max_frames)

    def update(self, frames, sample_base=0, levels=None, mlat=None, modes=None, commb=None, es=None):
        """frames: FRAME_DTYPE array in ascending offset (host); packet time = (sample_base + offset) x sps.  levels
        (after levels_reserve): the frames' LEVEL_DTYPE records (host), merged into the aircraft's level records.  mlat
        (after mlat_reserve): the frames' MLAT_FIX_DTYPE fixes (host), merged into the aircraft's mlat records.  modes
        (after modes_reserve): the frames' MODES_DTYPE records (host); the list is then keyed by their addresses, a
        frame that is not SELF or KNOWN touches nothing, and the aircraft's modes records take the replies.  commb
        (with modes, after commb_reserve): the frames' COMMB_DTYPE records (host); the aircraft's commb records take the
        registers, and a reply that reads as 5,0 and as 6,0 is settled against the aircraft's ADS-B velocity.  es (after
        es_reserve): the frames' ES_DTYPE records (host); the update is the one the other arguments choose, and the
        aircraft's es records take the extended squitter status, NIC and Rc of every position message resolved."""
        frames = np.ascontiguousarray(frames, dtype=FRAME_DTYPE)
        ptr = frames.ctypes.data if len(frames) else None
        if commb is not None and modes is None:
            raise ValueError("commb needs modes")
        if es is not None:
            n = len(frames)
            given = {"es": (es, ES_DTYPE), "modes": (modes, MODES_DTYPE), "commb": (commb, COMMB_DTYPE),
                     "mlat": (mlat, MLAT_FIX_DTYPE)}
            arrays = {}
            for name, (arr, dtype) in given.items():
                arrays[name] = None if arr is None else np.ascontiguousarray(arr, dtype=dtype)
                if arrays[name] is not None and len(arrays[name]) != n:
                    raise ValueError(f"{name}: {len(arrays[name])} records for {n} frames")
            keep, lptr = (None, None) if levels is None else self._host_levels(levels, n)
            at = lambda a: a.ctypes.data if a is not None and len(a) else None
            self._call("update_es", ptr, at(arrays["es"]), at(arrays["modes"]), at(arrays["commb"]), at(arrays["mlat"]),
                       lptr, n, int(sample_base))
            return
        if modes is not None:
            recs = np.ascontiguousarray(modes, dtype=MODES_DTYPE)
            if len(recs) != len(frames):
                raise ValueError(f"modes: {len(recs)} records for {len(frames)} frames")
            fixes = None if mlat is None else np.ascontiguousarray(mlat, dtype=MLAT_FIX_DTYPE)
            if fixes is not None and len(fixes) != len(frames):
                raise ValueError(f"mlat: {len(fixes)} fixes for {len(frames)} frames")
            keep, lptr = (None, None) if levels is None else self._host_levels(levels, len(frames))
            fptr = fixes.ctypes.data if fixes is not None and len(fixes) else None
            if commb is not None:
                cb = np.ascontiguousarray(commb, dtype=COMMB_DTYPE)
                if len(cb) != len(frames):
                    raise ValueError(f"commb: {len(cb)} records for {len(frames)} frames")
                self._call("update_commb", ptr, recs.ctypes.data if len(recs) else None,
                           cb.ctypes.data if len(cb) else None, fptr, lptr, len(frames), int(sample_base))
            else:
                self._call("update_modes", ptr, recs.ctypes.data if len(recs) else None, fptr, lptr, len(frames),
                           int(sample_base))
        elif mlat is not None:
            fixes = np.ascontiguousarray(mlat, dtype=MLAT_FIX_DTYPE)
            if len(fixes) != len(frames):
                raise ValueError(f"mlat: {len(fixes)} fixes for {len(frames)} frames")
            keep, lptr = (None, None) if levels is None else self._host_levels(levels, len(frames))
            self._call("update_mlat", ptr, fixes.ctypes.data if len(fixes) else None, lptr, len(frames), int(sample_base))
        elif levels is None:
            self._call("update", ptr, len(frames), int(sample_base))
        else:
            keep, lptr = self._host_levels(levels, len(frames))
            self._call("update_levels", ptr, lptr, len(frames), int(sample_base))

    def update_device(self, dev_ptr, n, sample_base=0, levels_ptr=None, mlat_ptr=None, modes_ptr=None, commb_ptr=None,
                      es_ptr=None):
        """n frames at dev_ptr in the ctx device's memory (e.g. result_device() after fetch_counts()).  levels_ptr
        (after levels_reserve): their n level records, on the device (e.g. levels_device()) or a host address.  mlat_ptr
        (after mlat_reserve): their n adsb_mlat_fix records, on the device (e.g. mlat_device()[0]) or a host address;
        every address may be a host one too, each on its own.  modes_ptr (after modes_reserve): their n adsb_modes_rec
        records (e.g. modes_device()[0]); the update is then update_modes.  commb_ptr (with modes_ptr, after
        commb_reserve): their n adsb_commb_rec records (e.g. commb_device()[0]); the update is then update_commb.  es_ptr
        (after es_reserve): their n adsb_es_rec records (e.g. es_device()[0]); the update the other arguments choose is
        then made through update_es."""
        if es_ptr is not None:
            if commb_ptr is not None and modes_ptr is None:
                raise ValueError("commb_ptr needs modes_ptr")
            self._call("update_es", dev_ptr, es_ptr, modes_ptr, commb_ptr, mlat_ptr, levels_ptr, int(n), int(sample_base))
        elif commb_ptr is not None:
            if modes_ptr is None:
                raise ValueError("commb_ptr needs modes_ptr")
            self._call("update_commb", dev_ptr, modes_ptr, commb_ptr, mlat_ptr, levels_ptr, int(n), int(sample_base))
        elif modes_ptr is not None:
            self._call("update_modes", dev_ptr, modes_ptr, mlat_ptr, levels_ptr, int(n), int(sample_base))
        elif mlat_ptr is not None:
            self._call("update_mlat", dev_ptr, mlat_ptr, levels_ptr, int(n), int(sample_base))
        elif levels_ptr is None:
            self._call("update", dev_ptr, int(n), int(sample_base))
        else:
            self._call("update_levels", dev_ptr, levels_ptr, int(n), int(sample_base))

    def levels(self):
        """AIRCRAFT_LEVEL_DTYPE records (each aircraft's signal level), aligned with aircraft()[0]."""
        return self._fetch("fetch_levels", [AIRCRAFT_LEVEL_DTYPE])[0]

    def mlat_reserve(self, max_disagreement_m):
        """adsb_track_table_mlat_reserve: one AIRCRAFT_MLAT_DTYPE record beside every aircraft record, which an update
        given `mlat` merges the frames' fixes into; a reported airborne position farther than max_disagreement_m (metres)
        from the solved one disagrees."""
        self._call("mlat_reserve", float(max_disagreement_m))

    def mlat(self):
        """AIRCRAFT_MLAT_DTYPE records (each aircraft's newest multilaterated position and its check counts), aligned
        with aircraft()[0]."""
        return self._fetch("fetch_mlat", [AIRCRAFT_MLAT_DTYPE])[0]

    def frame_mlat(self):
        """One FRAME_MLAT_DTYPE record per frame of the last update given `mlat`, in its list order."""
        return self._fetch("fetch_frame_mlat", [FRAME_MLAT_DTYPE], size=self.max_frames)[0]

    def mlat_device(self):
        """Device address of the mlat records, one per record place in slot order (as levels_device); no
        synchronisation."""
        dev = C.c_void_p()
        self._call("mlat_device", C.byref(dev))
        return dev.value

    def filter_reserve(self, **cfg):
        """adsb_track_table_filter_reserve (after mlat_reserve): one AIRCRAFT_FILTER_DTYPE record beside every aircraft
        record; every update given `mlat` then also runs each aircraft's fixes through a Kalman filter (position and
        velocity on north, east and up).  cfg: FILTER_CFG_FIELDS, each 0 or absent for its default."""
        c = _filter_cfg(**cfg)
        self._call("filter_reserve", C.byref(c))

    def filter(self):
        """AIRCRAFT_FILTER_DTYPE records (each aircraft's filtered mlat track), aligned with aircraft()[0];
        filter_physical() gives speed, track and vertical rate."""
        return self._fetch("fetch_filter", [AIRCRAFT_FILTER_DTYPE])[0]

    def frame_filter(self):
        """One FRAME_FILTER_DTYPE record per frame of the last update given `mlat`, in its list order: the aircraft's
        filtered position right after the frame, its nis and what the filter did with it."""
        return self._fetch("fetch_frame_filter", [FRAME_FILTER_DTYPE], size=self.max_frames)[0]

    def filter_device(self):
        """Device address of the filter records, one per record place in slot order (as levels_device); no
        synchronisation."""
        dev = C.c_void_p()
        self._call("filter_device", C.byref(dev))
        return dev.value

    def filter_operands(self):
        """adsb_debug_track_filter_operands: the FILTER_OPERAND_DTYPE records of the last update given `mlat`, in SORTED
        order (ascending address, list order within one).  For tests."""
        n = C.c_size_t()
        out = np.zeros(max(self.max_frames, 1), dtype=FILTER_OPERAND_DTYPE)
        L.check(self._lib.adsb_debug_track_filter_operands(self._h, out.ctypes.data_as(C.POINTER(L.AdsbFilterOperand)),
                                                           len(out), C.byref(n)), "adsb_debug_track_filter_operands")
        return out[:n.value].copy()

    def modes_reserve(self):
        """adsb_track_table_modes_reserve: one AIRCRAFT_MODES_DTYPE record beside every aircraft record, which an update
        given `modes` merges the frames' Mode S records into."""
        self._call("modes_reserve")

    def modes(self):
        """AIRCRAFT_MODES_DTYPE records (what each aircraft's Mode S replies say), aligned with aircraft()[0]."""
        return self._fetch("fetch_modes", [AIRCRAFT_MODES_DTYPE])[0]

    def modes_device(self):
        """Device address of the modes records, one per record place in slot order (as levels_device); no
        synchronisation."""
        dev = C.c_void_p()
        self._call("modes_device", C.byref(dev))
        return dev.value

    def commb_reserve(self, max_age_s=10.0, max_speed_diff_kt=40, max_vrate_diff_fpm=1000):
        """adsb_track_table_commb_reserve: one AIRCRAFT_COMMB_DTYPE record beside every aircraft record, which an update
        given `modes` and `commb` merges the frames' Comm-B registers into.  An ambiguous {5,0; 6,0} reply is settled
        against the aircraft's airborne velocity if that is at most max_age_s old, with these tolerances."""
        cfg = L.AdsbCommbSettleCfg(float(max_age_s), int(max_speed_diff_kt), int(max_vrate_diff_fpm))
        self._call("commb_reserve", C.byref(cfg))

    def commb(self):
        """AIRCRAFT_COMMB_DTYPE records (what each aircraft's Comm-B replies say), aligned with aircraft()[0];
        aircraft_commb_physical() gives them in physical units."""
        return self._fetch("fetch_commb", [AIRCRAFT_COMMB_DTYPE])[0]

    def frame_commb(self):
        """One COMMB_DTYPE record per frame of the last update given `commb`, in its list order: the frame's record,
        with state COMMB_SETTLED and the settled register's values where the table settled it."""
        return self._fetch("fetch_frame_commb", [COMMB_DTYPE], size=self.max_frames)[0]

    def commb_device(self):
        """Device address of the commb records, one per record place in slot order (as levels_device); no
        synchronisation."""
        dev = C.c_void_p()
        self._call("commb_device", C.byref(dev))
        return dev.value

    def es_reserve(self, max_age_s=60.0):
        """adsb_track_table_es_reserve: one AIRCRAFT_ES_DTYPE record beside every aircraft record, which an update given
        `es` merges the frames' extended squitter status into.  A position message's NIC and Rc are resolved with the
        aircraft's version and with NIC supplements A and C that are at most max_age_s old (policy, not a measurement;
        float("inf") keeps them for ever)."""
        cfg = L.AdsbEsTrackCfg(float(max_age_s))
        self._call("es_reserve", C.byref(cfg))

    def es(self):
        """AIRCRAFT_ES_DTYPE records (what each aircraft's extended squitters say, NIC and Rc resolved), aligned with
        aircraft()[0]; aircraft_es_physical() gives them in physical units."""
        return self._fetch("fetch_es", [AIRCRAFT_ES_DTYPE])[0]

    def frame_es(self):
        """One FRAME_INTEGRITY_DTYPE record per frame of the last update given `es`, in its list order: NIC and Rc of a
        position message as resolved, the version known before the frame, and the COUNTED / POSITION / VERSIONED /
        STALE flags; all zero for a frame that was not counted."""
        return self._fetch("fetch_frame_es", [FRAME_INTEGRITY_DTYPE], size=self.max_frames)[0]

    def es_device(self):
        """Device address of the es records, one per record place in slot order (as levels_device); no
        synchronisation."""
        dev = C.c_void_p()
        self._call("es_device", C.byref(dev))
        return dev.value

    def fixes_reserve(self, site):
        """adsb_track_table_fixes_reserve: from now on every update also decodes each position message on its own
        against `site` ((latitude, longitude[, max_range_nm = 180]) or a SITE record) and keeps the newest fix per
        aircraft.  The table must hold no aircraft."""
        self._fixes_reserve(site.reshape(-1) if isinstance(site, np.ndarray) else [site], 1)

    def fixes(self):
        """FIX_DTYPE records (each aircraft's newest single-message position, with range and bearing from the site),
        aligned with aircraft()[0]."""
        return self._fetch("fetch_fixes", [FIX_DTYPE])[0]

    def aircraft(self):
        """(AIRCRAFT_DTYPE records of the whole table in ascending ICAO, table flags)."""
        flags = C.c_uint32()
        recs, = self._fetch("fetch", [AIRCRAFT_DTYPE], (C.byref(flags),), (C.byref(flags),))
        return recs, flags.value

    def expire(self, before):
        """Evicts every aircraft whose last frame of any kind is older than `before` seconds (asynchronous)."""
        self._call("expire", float(before))

    def last_heard(self):
        """float64 last-heard times (seconds), aligned with aircraft()[0]."""
        return self._fetch("fetch_last_heard", [np.float64])[0]

    def velocity(self):
        """VELOCITY_DTYPE records (each aircraft's last airborne-velocity message), aligned with aircraft()[0]."""
        return self._fetch("fetch_velocity", [VELOCITY_DTYPE])[0]

    def changed(self):
        """(records, last_heard, velocity) of the aircraft the last update touched, ascending ICAO: the matching rows
        of aircraft()[0], last_heard() and velocity(), without copying the table."""
        return tuple(self._fetch("fetch_changed", [AIRCRAFT_DTYPE, np.float64, VELOCITY_DTYPE]))


class TrackBank(_TrackStore):
    """adsb_track_bank_*: n_receivers independent aircraft tables on the device (one HashMap<u32, Aircraft> per
    receiver's display thread), all updated by one call over a multi-receiver frame list; receiver r equals a
    TrackTable fed receiver r's part of every update."""
    _prefix = "adsb_track_bank_"

    def __init__(self, dem, n_receivers, max_aircraft=0, max_frames=1 << 16, seconds_per_sample=0.5e-6):
        self._open(dem, L.AdsbTrackBankCfg(L.ADSB_ABI_VERSION, int(n_receivers), int(max_aircraft), 0, int(max_frames),
                                           float(seconds_per_sample)), max_frames)
        self.n_receivers = int(n_receivers)
        self._fuse_reserved = None       # max_fused of the last fuse_reserve

    def _u64s(self, values, what):
        """None / a scalar (the same for every receiver) / a per-receiver sequence -> a uint64[n_receivers] array."""
        if values is None:
            return None
        if np.ndim(values) == 0:
            values = [int(values)] * self.n_receivers
        values = [int(v) for v in values]
        if len(values) != self.n_receivers:
            raise ValueError(f"{what}: {len(values)} values for {self.n_receivers} receivers")
        return (C.c_uint64 * self.n_receivers)(*values)

    def _split(self, out, counts):
        """One array of all receivers' rows -> a list of n_receivers arrays, counts[r] rows each."""
        edges = np.concatenate([[0], np.cumsum(list(counts))]).astype(np.int64)
        return [out[edges[r]:edges[r + 1]].copy() for r in range(self.n_receivers)]

    def update(self, frames, counts, sample_base=None, levels=None):
        """frames: FRAME_DTYPE array (host), receiver 0's frames in ascending offset, then receiver 1's, ...;
        counts: frames of each receiver; sample_base: scalar or per receiver (frame time = (base + offset) x sps);
        levels (after levels_reserve): the frames' LEVEL_DTYPE records (host), merged into the level records."""
        frames = np.ascontiguousarray(frames, dtype=FRAME_DTYPE)
        ptr = frames.ctypes.data if len(frames) else None
        split = (self._u64s(counts, "counts"), self._u64s(sample_base, "sample_base"))
        if levels is None:
            self._call("update", ptr, len(frames), *split)
        else:
            keep, lptr = self._host_levels(levels, len(frames))
            self._call("update_levels", ptr, lptr, len(frames), *split)

    def update_device(self, dev_ptr, n, counts, sample_base=None, levels_ptr=None):
        """n frames at dev_ptr in the ctx device's memory, split by counts as for update().  levels_ptr (after
        levels_reserve): their n level records, on the device or a host address."""
        split = (self._u64s(counts, "counts"), self._u64s(sample_base, "sample_base"))
        if levels_ptr is None:
            self._call("update", dev_ptr, int(n), *split)
        else:
            self._call("update_levels", dev_ptr, levels_ptr, int(n), *split)

    def update_launch(self, sample_base=None, levels=False):
        """The ctx's last launch, channel k -> receiver k: what fetch() returns, read in device memory.  levels=True
        (after levels_reserve): with the launch's levels, which are enqueued here if they have not been."""
        self._call("update_launch_levels" if levels else "update_launch", self._u64s(sample_base, "sample_base"))

    def aircraft(self):
        """(list of n_receivers AIRCRAFT_DTYPE arrays, each in ascending ICAO; list of per-receiver flags)."""
        counts = (C.c_uint64 * self.n_receivers)()
        flags = (C.c_uint32 * self.n_receivers)()
        out, = self._fetch("fetch", [AIRCRAFT_DTYPE], (None, None), (counts, flags))
        return self._split(out, counts), list(flags)

    def expire(self, before):
        """Evicts, on every receiver r, the aircraft whose last frame is older than before[r] seconds; `before` is a
        scalar (the same for every receiver) or a per-receiver sequence (-inf: keep all).  Asynchronous."""
        if np.ndim(before) == 0:
            before = [float(before)] * self.n_receivers
        before = [float(v) for v in before]
        if len(before) != self.n_receivers:
            raise ValueError(f"before: {len(before)} values for {self.n_receivers} receivers")
        self._call("expire", (C.c_double * self.n_receivers)(*before))

    def _aligned(self, name, dtype):
        """fetch_last_heard / fetch_velocity as a list of n_receivers arrays, aligned with aircraft()[0]."""
        sizes = [len(x) for x in self.aircraft()[0]]      # the per-receiver split of the same records
        return self._split(self._fetch(name, [dtype], size=sum(sizes))[0], sizes)

    def last_heard(self):
        """list of n_receivers float64 arrays of last-heard times (seconds), aligned with aircraft()[0]."""
        return self._aligned("fetch_last_heard", np.float64)

    def velocity(self):
        """list of n_receivers VELOCITY_DTYPE arrays, aligned with aircraft()[0]."""
        return self._aligned("fetch_velocity", VELOCITY_DTYPE)

    def levels(self):
        """list of n_receivers AIRCRAFT_LEVEL_DTYPE arrays, aligned with aircraft()[0]."""
        return self._aligned("fetch_levels", AIRCRAFT_LEVEL_DTYPE)

    def fixes_reserve(self, sites):
        """adsb_track_bank_fixes_reserve: as TrackTable.fixes_reserve with one site per receiver (a SITE array or a
        sequence of (latitude, longitude[, max_range_nm = 180]))."""
        self._fixes_reserve(sites, self.n_receivers)

    def fixes(self):
        """list of n_receivers FIX_DTYPE arrays, aligned with aircraft()[0]."""
        return self._aligned("fetch_fixes", FIX_DTYPE)

    def fused_levels(self):
        """FUSED_LEVEL_DTYPE records of the last fuse_async() / fuse(), one per fused record in the same order; needs
        both fuse_reserve and levels_reserve before that fuse."""
        return self._fetch("fetch_fused_levels", [FUSED_LEVEL_DTYPE])[0]

    def fuse(self, since=-math.inf, max_fused=None):
        """The fused view: one FUSED_DTYPE record per distinct ICAO over all receivers, ascending ICAO, from the records
        with last_heard >= since.  Reserves on first use and whenever max_fused changes (None: as reserved before, or
        n_receivers x max_aircraft), fuses on the device and fetches.  Returns (records, n_total, flags): n_total counts
        the distinct ICAOs even when they exceed max_fused, and flags then has ADSB_TRACK_FUSED_TRUNCATED."""
        want = 0 if max_fused is None else int(max_fused)
        if want < 0:
            raise ValueError("max_fused must be positive, or None")
        if self._fuse_reserved is None or (max_fused is not None and want != self._fuse_reserved):
            self.fuse_reserve(want)
        self.fuse_async(since)
        n, total, flags = C.c_size_t(), C.c_size_t(), C.c_uint32()
        self._call("fetch_fused", None, 0, C.byref(n), C.byref(total), C.byref(flags))
        out = np.zeros(max(total.value, 1), dtype=FUSED_DTYPE)
        self._call("fetch_fused", out.ctypes.data_as(C.POINTER(L.AdsbFusedAircraft)), len(out), C.byref(n),
                   C.byref(total), C.byref(flags))
        return out[:n.value].copy(), int(total.value), int(flags.value)

    def fuse_reserve(self, max_fused=0):
        """adsb_track_bank_fuse_reserve: memory for up to max_fused fused records (0: n_receivers x max_aircraft)."""
        self._call("fuse_reserve", int(max_fused))
        self._fuse_reserved = int(max_fused)

    def fuse_async(self, since=-math.inf):
        """adsb_track_bank_fuse alone: enqueues the fusion on the ctx stream (after fuse_reserve) and returns."""
        self._call("fuse", float(since))

    def fused_device(self):
        """(device address of the fused records, device address of uint64[2]: records written, distinct ICAOs) of the
        last fuse, for consumers that stay on the GPU; valid on the ctx stream, no synchronisation."""
        rec, counts = C.c_void_p(), C.c_void_p()
        self._call("fused_device", C.byref(rec), C.byref(counts))
        return rec.value, counts.value

    def changed(self):
        """(records, last_heard, velocity, per-receiver counts) of the aircraft the last update touched: receiver 0's in
        ascending ICAO, then receiver 1's, ...; rows of aircraft(), last_heard() and velocity()."""
        counts = (C.c_uint64 * self.n_receivers)()
        rows = self._fetch("fetch_changed", [AIRCRAFT_DTYPE, np.float64, VELOCITY_DTYPE], (None,), (counts,))
        return (*rows, [int(x) for x in counts])


def packet_new(frame_bytes):
    """AdsbPacket::new (packet.rs:25-49) -> AdsbPacketView."""
    b = (C.c_uint8 * 14)(*bytes(frame_bytes))
    v = L.AdsbPacketView()
    L.check(L.load().adsb_packet_new(C.byref(b), C.byref(v)), "adsb_packet_new")
    return v


def packet_new_from_string(hexstr):
    v = L.AdsbPacketView()
    L.check(L.load().adsb_packet_new_from_string(hexstr.encode(), C.byref(v)),
            "adsb_packet_new_from_string")
    return v


def packet_display(frame_bytes, time_text=""):
    b = (C.c_uint8 * 14)(*bytes(frame_bytes))
    buf = C.create_string_buffer(2048)
    n = L.load().adsb_packet_display(C.byref(b), time_text.encode(), buf, 2048)
    return buf.value.decode()[:n]
