"""ctypes binding of libadsb_hip.so (include/adsb_hip.h, include/adsb_host.h).

There is no CPU fallback: if the HIP library has not been built this module raises, and without
a HIP device ``adsb_create`` returns ADSB_E_NODEVICE.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# ADSB_HIP_LIB lets tuning experiments point at another build of the same library
LIB_PATH = os.environ.get("ADSB_HIP_LIB") or os.path.join(_HERE, "lib", "libadsb_hip.so")

ADSB_ABI_VERSION = 1
ADSB_OK = 0
ADSB_E_SHORT = -1
ADSB_E_ARG = -2
ADSB_E_CAPACITY = -3
ADSB_E_NOMEM = -4
ADSB_E_NODEVICE = -5
ADSB_E_STATE = -6
ADSB_FLAG_TRUNCATED = 0x1
ADSB_FLAG_INCOMPLETE = 0x2
ADSB_SAMPLE_I8 = 0
ADSB_SAMPLE_I16 = 1
ADSB_MSG_AIRCRAFT_ID, ADSB_MSG_AIRCRAFT_POSITION, ADSB_MSG_UNKNOWN = 0, 1, 2
ADSB_REPLAY_CARRY, ADSB_REPLAY_SEND_TAIL = 0x1, 0x2
ADSB_FILE_C16, ADSB_FILE_U8 = 0, 1


class AdsbFrame(C.Structure):
    _fields_ = [("offset", C.c_uint64), ("bytes", C.c_uint8 * 14), ("status", C.c_uint8),
                ("fixed_bit", C.c_uint8)]


class AdsbCfg(C.Structure):
    _fields_ = [("abi_version", C.c_uint32), ("device", C.c_int32), ("sample_type", C.c_int32),
                ("max_channels", C.c_uint32), ("max_samples", C.c_uint64), ("max_out", C.c_uint64),
                ("stream", C.c_void_p), ("host_staging", C.c_uint32), ("reserved", C.c_uint32)]


class AdsbFeedCfg(C.Structure):
    _fields_ = [("max_chunk", C.c_size_t), ("carry", C.c_uint32), ("ring_slots", C.c_uint32)]


class AdsbGroupCfg(C.Structure):
    _fields_ = [("abi_version", C.c_uint32), ("sample_type", C.c_int32), ("n_members", C.c_uint32), ("root", C.c_uint32),
                ("devices", C.POINTER(C.c_int32)), ("max_samples", C.c_uint64), ("max_out", C.c_uint64),
                ("host_staging", C.c_uint32), ("reserved", C.c_uint32)]


class AdsbGroupShard(C.Structure):
    _fields_ = [("first_sample", C.c_uint64), ("n_samples", C.c_uint64), ("n_offsets", C.c_uint64)]


class AdsbSynthCfg(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("slot_len", C.c_uint32), ("frame_pct", C.c_uint32),
                ("pct_flip_data", C.c_uint32), ("pct_flip_crc", C.c_uint32),
                ("pct_flip_two", C.c_uint32), ("noise_div", C.c_uint32), ("amp_shift", C.c_uint32),
                ("reserved", C.c_uint32)]


class AdsbPacketFields(C.Structure):
    _fields_ = [("icao", C.c_uint32), ("altitude", C.c_int32), ("cpr_latitude", C.c_uint32),
                ("cpr_longitude", C.c_uint32), ("downlink_format", C.c_uint8), ("capability", C.c_uint8),
                ("msg_type", C.c_uint8), ("msg_kind", C.c_uint8), ("surveillance_status", C.c_uint8),
                ("nic_supplement", C.c_uint8), ("cpr_time", C.c_uint8), ("cpr_odd", C.c_uint8),
                ("callsign", C.c_char * 8)]


ADSB_LEVEL_VALID = 0x1  # adsb_frame_level.flags: the frame's window lay inside the buffer
ADSB_LEVEL_SHORT = 0x2  # ... and it is a 56-bit frame's record: sums over 60 and 68 samples (adsb_levels_modes_of)


class AdsbFrameLevel(C.Structure):
    _fields_ = [("signal_sum", C.c_uint64), ("noise_sum", C.c_uint64), ("peak", C.c_uint32), ("pulse_min", C.c_uint32),
                ("quiet_max", C.c_uint32), ("weak_bits", C.c_uint16), ("flags", C.c_uint16)]


ADSB_WIRE_BEAST, ADSB_WIRE_AVR, ADSB_WIRE_AVR_MLAT = 0, 1, 2  # adsb_wire_cfg.format
ADSB_WIRE_SHORT = 0x100                                      # ... a bit of it: 56-bit frames leave as short frames
ADSB_WIRE_MAX_BYTES = 44                                     # the longest encoded frame (Beast, every byte doubled)


class AdsbWireCfg(C.Structure):
    """adsb_wire_cfg: format, whether Beast carries the signal byte, and the constant added to 6 x offset."""
    _fields_ = [("format", C.c_uint32), ("signal", C.c_uint32), ("tick_bias", C.c_uint64)]


ADSB_WIRE_IN_CRC, ADSB_WIRE_IN_DF17, ADSB_WIRE_IN_SHORT = 0x1, 0x2, 0x4   # adsb_wire_in_cfg.filter


class AdsbWireInCfg(C.Structure):
    """adsb_wire_in_cfg: what adsb_wire_in_of / adsb_host_wire_parse read and keep."""
    _fields_ = [("format", C.c_uint32), ("filter", C.c_uint32), ("tick_bias", C.c_uint64), ("max_frames", C.c_uint64),
                ("sample_type", C.c_int32), ("levels", C.c_uint32)]


class AdsbWireRx(C.Structure):
    """adsb_wire_rx: how one parsed frame arrived (16 bytes)."""
    _fields_ = [("ticks", C.c_uint64), ("pos", C.c_uint32), ("signal", C.c_uint8), ("kind", C.c_uint8),
                ("receiver", C.c_uint16)]


class AdsbWireInHeader(C.Structure):
    """adsb_wire_in_header: the totals of one parse (64 bytes)."""
    _fields_ = [(k, C.c_uint64) for k in ("n_frames", "total_found", "n_marks", "n_cut", "n_unknown", "n_other",
                                          "n_rejected", "flags")]


ADSB_MODES_SELF, ADSB_MODES_KNOWN, ADSB_MODES_UNKNOWN, ADSB_MODES_PARITY, ADSB_MODES_UNSUPPORTED = 0, 1, 2, 3, 4
(ADSB_MODES_ALT, ADSB_MODES_ALT_METRIC, ADSB_MODES_SQUAWK, ADSB_MODES_GROUND, ADSB_MODES_ALERT, ADSB_MODES_SPI,
 ADSB_MODES_CALLSIGN) = 0x1, 0x2, 0x4, 0x8, 0x10, 0x20, 0x40    # adsb_modes_rec.flags


class AdsbModesRec(C.Structure):
    """adsb_modes_rec: one frame's address, kind and surveillance fields (32 bytes)."""
    _fields_ = [("address", C.c_uint32), ("df", C.c_uint8), ("kind", C.c_uint8), ("flags", C.c_uint16),
                ("altitude_ft", C.c_int32), ("squawk", C.c_uint16), ("fs", C.c_uint8), ("dr", C.c_uint8),
                ("um", C.c_uint8), ("iid", C.c_uint8), ("ca", C.c_uint8), ("ri", C.c_uint8), ("callsign", C.c_char * 8),
                ("reserved", C.c_uint8 * 4)]


class AdsbModesHeader(C.Structure):
    """adsb_modes_header: the totals of one adsb_modes_of (64 bytes)."""
    _fields_ = [(k, C.c_uint64) for k in ("n", "n_self", "n_known", "n_unknown", "n_parity", "n_unsupported",
                                          "n_known_out", "n_squitters")]


(ADSB_COMMB_NOT_COMMB, ADSB_COMMB_EMPTY, ADSB_COMMB_NONE, ADSB_COMMB_ONE,
 ADSB_COMMB_AMBIGUOUS) = 0, 1, 2, 3, 4                          # adsb_commb_rec.state
(ADSB_COMMB_C10, ADSB_COMMB_C17, ADSB_COMMB_C20, ADSB_COMMB_C30, ADSB_COMMB_C40, ADSB_COMMB_C50,
 ADSB_COMMB_C60) = 0x1, 0x2, 0x4, 0x8, 0x10, 0x20, 0x40         # adsb_commb_rec.candidates


class AdsbCommbRec(C.Structure):
    """adsb_commb_rec: the Comm-B register one DF20/21 frame carries, and its values (32 bytes)."""
    _fields_ = [("state", C.c_uint8), ("bds", C.c_uint8), ("candidates", C.c_uint8), ("n_candidates", C.c_uint8),
                ("status", C.c_uint16), ("reserved", C.c_uint16), ("value", C.c_int32 * 5), ("word", C.c_uint32)]


class AdsbCommbHeader(C.Structure):
    """adsb_commb_header: the totals of one adsb_commb_of (128 bytes)."""
    _fields_ = ([(k, C.c_uint64) for k in ("n", "n_commb", "n_empty", "n_none", "n_one", "n_ambiguous")]
                + [("n_bds", C.c_uint64 * 7), ("reserved", C.c_uint64 * 3)])


(ADSB_ES_NOT_ES, ADSB_ES_FOREIGN, ADSB_ES_CATEGORY, ADSB_ES_POSITION, ADSB_ES_VELOCITY, ADSB_ES_EMERGENCY, ADSB_ES_ACAS_RA,
 ADSB_ES_TARGET_STATE, ADSB_ES_OPERATIONAL, ADSB_ES_RESERVED) = range(10)                       # adsb_es_rec.state
ES_PRESENT = ("CATEGORY", "NIC_B", "RC", "NAC_V", "VELOCITY_FLAGS", "EMERGENCY", "SQUAWK", "RA", "SIL_SUPPLEMENT", "ALT_SOURCE",
              "SELECTED_ALT", "BARO", "HEADING", "NAC_P", "NIC_BARO", "SIL", "MODES", "TCAS", "VERSION", "CC_OM", "NIC_A", "HRD",
              "TRACK_HEADING", "LENGTH_WIDTH", "SDA", "GVA", "NIC_C")                            # adsb_es_rec.present, bit k
ES_FLAGS = ("INTENT_CHANGE", "IFR", "ALT_FMS", "AUTOPILOT", "VNAV", "ALT_HOLD", "APPROACH", "LNAV", "TCAS", "HRD",
            "TRACK_HEADING")                                                                    # adsb_es_rec.flags, bit k
globals().update({"ADSB_ES_HAS_" + name: 1 << k for k, name in enumerate(ES_PRESENT)})
globals().update({"ADSB_ES_" + name: 1 << k for k, name in enumerate(ES_FLAGS)})
ADSB_ES_VERSION_UNKNOWN = 0xFF


class AdsbEsRec(C.Structure):
    """adsb_es_rec: what one DF17/18 frame says about the aircraft's status (32 bytes)."""
    _fields_ = ([("state", C.c_uint8), ("type_code", C.c_uint8), ("subtype", C.c_uint8), ("version", C.c_uint8),
                 ("present", C.c_uint32)]
                + [(k, C.c_uint8) for k in ("nic_a", "nic_b", "nic_c", "nac_p", "nac_v", "sil", "sil_supplement", "gva", "sda",
                                            "nic_baro", "category", "emergency", "length_width", "reserved")]
                + [("flags", C.c_uint16), ("value", C.c_uint32), ("half", C.c_uint16 * 2)])


class AdsbEsHeader(C.Structure):
    """adsb_es_header: the totals of one adsb_es_of (128 bytes)."""
    _fields_ = [("n", C.c_uint64), ("n_state", C.c_uint64 * 10), ("n_version", C.c_uint64 * 4), ("reserved", C.c_uint64)]


ADSB_REPLIES_AP_KNOWN = 0x1        # adsb_replies_cfg.flags
ADSB_MERGE_FROM_B = 0x80000000     # src[] of a merge: the frame is list B's


class AdsbRepliesCfg(C.Structure):
    """adsb_replies_cfg: the filter, the capacity and the stream position of one adsb_replies_of (32 bytes)."""
    _fields_ = [("flags", C.c_uint32), ("reserved", C.c_uint32), ("max_frames", C.c_uint64),
                ("first_sample_index", C.c_uint64), ("reserved2", C.c_uint64)]


class AdsbRepliesHeader(C.Structure):
    """adsb_replies_header: the totals of one adsb_replies_of (80 bytes)."""
    _fields_ = [(k, C.c_uint64) for k in ("n_out", "total_found", "n_preamble", "n_all_call", "n_df18", "n_address_parity",
                                          "n_not_known", "n_parity", "flags", "reserved")]


assert C.sizeof(AdsbRepliesCfg) == 32 and C.sizeof(AdsbRepliesHeader) == 80


class AdsbCorrelateCfg(C.Structure):
    """adsb_correlate_cfg: the window in samples, and whether adsb_correlate_launch takes the launch's levels."""
    _fields_ = [("window", C.c_uint32), ("use_levels", C.c_uint32), ("reserved", C.c_uint64)]


class AdsbMessage(C.Structure):
    """adsb_message: one transmission, however many receivers heard it (64 bytes)."""
    _fields_ = [("time", C.c_uint64), ("bytes", C.c_uint8 * 14), ("status", C.c_uint8), ("fixed_bit", C.c_uint8),
                ("first", C.c_uint32), ("n_receptions", C.c_uint32), ("n_receivers", C.c_uint16),
                ("first_receiver", C.c_uint16), ("best_receiver", C.c_uint16), ("reserved", C.c_uint16),
                ("n_clean", C.c_uint32), ("reserved2", C.c_uint32), ("span", C.c_uint64),
                ("best_signal_sum", C.c_uint64)]


class AdsbReception(C.Structure):
    """adsb_reception: one receiver's hearing of a message (16 bytes)."""
    _fields_ = [("time", C.c_uint64), ("frame", C.c_uint32), ("receiver", C.c_uint16), ("reserved", C.c_uint16)]


ADSB_MLAT_C = 299792458.0 / 1.0003                           # propagation in air, m/s
ADSB_MLAT_MAX_RECEPTIONS = 256
ADSB_MLAT_TIME_RECEPTION, ADSB_MLAT_TIME_TICKS = 0, 1         # adsb_mlat_cfg.time_source
ADSB_MLAT_USE_ALTITUDE = 0x1                                 # adsb_mlat_cfg.flags
ADSB_MLAT_ATTEMPTED, ADSB_MLAT_CONVERGED, ADSB_MLAT_ALTITUDE, ADSB_MLAT_TOO_FEW = 0x1, 0x2, 0x4, 0x8  # adsb_mlat_fix.flags
ADSB_MLAT_TOO_MANY, ADSB_MLAT_SINGULAR, ADSB_MLAT_REJECTED_RESIDUAL, ADSB_MLAT_REJECTED_RANGE = 0x10, 0x20, 0x40, 0x80
ADSB_MLAT_VALID, ADSB_MLAT_BAD_INDEX = 0x100, 0x200
ADSB_MLAT_HDR_BAD_INDEX = 0x1                                # adsb_mlat_header.flags


class AdsbMlatReceiver(C.Structure):
    """adsb_mlat_receiver: WGS84 degrees, metres above the ellipsoid, and the clock's offset in seconds (32 bytes)."""
    _fields_ = [("latitude", C.c_double), ("longitude", C.c_double), ("height_m", C.c_double),
                ("clock_offset_s", C.c_double)]


class AdsbMlatCfg(C.Structure):
    """adsb_mlat_cfg: the time source, the altitude switch, and the solver's limits; 0 takes each default (64 bytes)."""
    _fields_ = [("time_source", C.c_uint32), ("flags", C.c_uint32), ("min_receivers", C.c_uint32),
                ("max_iterations", C.c_uint32), ("seconds_per_tick", C.c_double), ("step_tol_m", C.c_double),
                ("max_residual_m", C.c_double), ("max_range_m", C.c_double), ("default_altitude_m", C.c_double),
                ("reserved", C.c_uint64)]


class AdsbMlatFix(C.Structure):
    """adsb_mlat_fix: where one message was sent from (64 bytes)."""
    _fields_ = [("latitude", C.c_double), ("longitude", C.c_double), ("height_m", C.c_double), ("time_s", C.c_double),
                ("residual_rms_m", C.c_float), ("pdop", C.c_float), ("hdop", C.c_float), ("vdop", C.c_float),
                ("n_used", C.c_uint16), ("iterations", C.c_uint16), ("flags", C.c_uint32), ("reserved", C.c_uint64)]


class AdsbMlatHeader(C.Structure):
    """adsb_mlat_header: the totals of one multilaterate call (32 bytes)."""
    _fields_ = [(k, C.c_uint64) for k in ("n_messages", "n_attempted", "n_valid", "flags")]


MLAT_RECEIVER_DTYPE = np.dtype([("latitude", "<f8"), ("longitude", "<f8"), ("height_m", "<f8"), ("clock_offset_s", "<f8")])
MLAT_FIX_DTYPE = np.dtype([("latitude", "<f8"), ("longitude", "<f8"), ("height_m", "<f8"), ("time_s", "<f8"),
                           ("residual_rms_m", "<f4"), ("pdop", "<f4"), ("hdop", "<f4"), ("vdop", "<f4"), ("n_used", "<u2"),
                           ("iterations", "<u2"), ("flags", "<u4"), ("reserved", "<u8")])
assert MLAT_RECEIVER_DTYPE.itemsize == C.sizeof(AdsbMlatReceiver) == 32
assert MLAT_FIX_DTYPE.itemsize == C.sizeof(AdsbMlatFix) == 64 and C.sizeof(AdsbMlatCfg) == 64


ADSB_CLOCK_DRIFT = 0x1                                       # adsb_clock_cfg.flags
ADSB_CLOCK_REFERENCE, ADSB_CLOCK_REACHED, ADSB_CLOCK_HAS_DRIFT = 0x1, 0x2, 0x4   # adsb_clock.flags
ADSB_CLOCK_HDR_BAD_INDEX, ADSB_CLOCK_HDR_DRIFT_DROPPED, ADSB_CLOCK_HDR_SINGULAR = 0x1, 0x2, 0x4  # adsb_clock_header.flags


class AdsbClockCfg(C.Structure):
    """adsb_clock_cfg: the time source and units, the reference receiver, and the second pass's limit (64 bytes)."""
    _fields_ = [("time_source", C.c_uint32), ("flags", C.c_uint32), ("reference", C.c_uint32), ("min_rows", C.c_uint32),
                ("seconds_per_tick", C.c_double), ("seconds_per_time", C.c_double), ("max_residual_s", C.c_double),
                ("max_range_nm", C.c_double), ("reserved", C.c_uint64 * 2)]


class AdsbClockHeader(C.Structure):
    """adsb_clock_header: the totals of one clock-sync call (64 bytes)."""
    _fields_ = [(k, C.c_uint64) for k in ("n_messages", "n_eligible", "n_rows", "n_dropped", "n_reached", "flags")] + \
               [("reserved", C.c_uint64 * 2)]


CLOCK_DTYPE = np.dtype([("offset_s", "<f8"), ("fine_offset_s", "<f8"), ("drift", "<f8"), ("residual_rms_s", "<f4"),
                        ("n_rows", "<u4"), ("n_dropped", "<u4"), ("n_partners", "<u4"), ("flags", "<u4"),
                        ("reserved", "<u4", (5,))])
assert CLOCK_DTYPE.itemsize == 64 and C.sizeof(AdsbClockCfg) == 64 and C.sizeof(AdsbClockHeader) == 64


class AdsbTrackPoint(C.Structure):
    _fields_ = [("latitude", C.c_double), ("longitude", C.c_double), ("icao", C.c_uint32), ("flags", C.c_uint32)]


class AdsbAircraftRecord(C.Structure):
    _fields_ = [("latitude", C.c_double), ("longitude", C.c_double), ("last_contact", C.c_double),
                ("icao", C.c_uint32), ("altitude", C.c_int32), ("has_position", C.c_uint32),
                ("n_frames", C.c_uint32), ("callsign", C.c_char * 8)]


class AdsbAircraftSummary(C.Structure):
    _fields_ = [("icao", C.c_uint32), ("callsign", C.c_char * 9), ("altitude", C.c_int32),
                ("has_position", C.c_int32), ("latitude", C.c_double), ("longitude", C.c_double),
                ("last_contact", C.c_double)]


ADSB_TRACK_NEW_POSITION = 0x1
ADSB_TRACK_UNTRACKED = 0x2   # point flag: the frame's aircraft was turned away by a full table
ADSB_TRACK_TABLE_FULL = 0x1  # table flag: some aircraft was turned away since create / reset


class AdsbTrackTableCfg(C.Structure):
    _fields_ = [("abi_version", C.c_uint32), ("max_aircraft", C.c_uint32), ("max_frames", C.c_uint64),
                ("seconds_per_sample", C.c_double)]


ADSB_VELOCITY_SPEED = 0x1      # adsb_velocity.flags: speed_kt holds a value
ADSB_VELOCITY_DIRECTION = 0x2  # direction_deg holds a value
ADSB_VELOCITY_VRATE = 0x4      # vertical_rate_fpm holds a value


class AdsbVelocity(C.Structure):
    _fields_ = [("time", C.c_double), ("speed_kt", C.c_float), ("direction_deg", C.c_float),
                ("vertical_rate_fpm", C.c_int32), ("v_ew_kt", C.c_int16), ("v_ns_kt", C.c_int16),
                ("subtype", C.c_uint8), ("flags", C.c_uint8), ("vrate_baro", C.c_uint8), ("airspeed_tas", C.c_uint8),
                ("reserved", C.c_uint32)]


ADSB_FUSED_NONE = 0xFFFF            # adsb_fused_aircraft.*_receiver: no contributing record has that quantity
ADSB_TRACK_FUSED_TRUNCATED = 0x1    # fetch_fused flag: more distinct ICAOs than max_fused


class AdsbFusedAircraft(C.Structure):
    """adsb_fused_aircraft; `velocity` stands for the header's eleven fields velocity_time .. velocity_reserved, which
    are an adsb_velocity bit for bit."""
    _fields_ = [("latitude", C.c_double), ("longitude", C.c_double), ("position_time", C.c_double),
                ("last_contact", C.c_double), ("last_heard", C.c_double), ("n_frames", C.c_uint64),
                ("icao", C.c_uint32), ("altitude", C.c_int32), ("n_receivers", C.c_uint16),
                ("heard_receiver", C.c_uint16), ("contact_receiver", C.c_uint16), ("position_receiver", C.c_uint16),
                ("callsign_receiver", C.c_uint16), ("velocity_receiver", C.c_uint16), ("has_position", C.c_uint32),
                ("callsign", C.c_char * 8), ("velocity", AdsbVelocity), ("reserved", C.c_uint64 * 2)]


class AdsbAircraftLevel(C.Structure):
    """adsb_aircraft_level: an aircraft's signal level beside its record (tables and banks with a levels reserve)."""
    _fields_ = [("signal_total", C.c_uint64), ("noise_total", C.c_uint64), ("last_signal_sum", C.c_uint64),
                ("last_noise_sum", C.c_uint64), ("max_signal_sum", C.c_uint64), ("last_time", C.c_double),
                ("n_levels", C.c_uint32), ("peak", C.c_uint32), ("weak_bits_total", C.c_uint32),
                ("reserved", C.c_uint32)]


class AdsbFusedLevel(C.Structure):
    """adsb_fused_level: one per fused record, same order; `strongest` stands for the header's ten fields
    strongest_signal_total .. strongest_reserved, which are an adsb_aircraft_level bit for bit."""
    _fields_ = [("strongest", AdsbAircraftLevel), ("signal_total", C.c_uint64), ("noise_total", C.c_uint64),
                ("n_levels", C.c_uint64), ("strongest_receiver", C.c_uint16), ("level_receivers", C.c_uint16),
                ("reserved", C.c_uint32)]


ADSB_FIX_VALID = 0x1      # adsb_fix.flags / adsb_frame_fix.flags: the record holds a fix
ADSB_FIX_SURFACE = 0x2    # from a surface message (TC 5-8)
ADSB_FIX_ALT = 0x4        # altitude holds a value (TC 9-18)
ADSB_FIX_SPEED = 0x8      # ground_speed_kt holds a value
ADSB_FIX_TRACK = 0x10     # track_deg holds a value
ADSB_FIX_REJECTED = 0x20  # adsb_frame_fix.flags only: a position message turned away


class AdsbSite(C.Structure):
    """adsb_site: a receiver's position (degrees) and the greatest range (NM, (0, 180]) it accepts a fix at."""
    _fields_ = [("latitude", C.c_double), ("longitude", C.c_double), ("max_range_nm", C.c_double)]


class AdsbFix(C.Structure):
    """adsb_fix: an aircraft's newest single-message position beside its record (tables and banks with a fixes
    reserve)."""
    _fields_ = [("time", C.c_double), ("latitude", C.c_double), ("longitude", C.c_double), ("range_nm", C.c_float),
                ("bearing_deg", C.c_float), ("ground_speed_kt", C.c_float), ("track_deg", C.c_float),
                ("altitude", C.c_int32), ("n_fixes", C.c_uint32), ("n_rejected", C.c_uint32), ("type_code", C.c_uint8),
                ("flags", C.c_uint8), ("cpr_odd", C.c_uint8), ("reserved8", C.c_uint8), ("reserved", C.c_uint32)]


class AdsbFrameFix(C.Structure):
    _fields_ = [("latitude", C.c_double), ("longitude", C.c_double), ("range_nm", C.c_float),
                ("bearing_deg", C.c_float), ("icao", C.c_uint32), ("flags", C.c_uint32)]


SITE = np.dtype([("latitude", "<f8"), ("longitude", "<f8"), ("max_range_nm", "<f8")])
# the struct's fields, and its 4 bytes of tail padding (zero) as a field of their own, so that every copy of a record
# carries all 64 bytes and tobytes() is the C record
FIX_DTYPE = np.dtype([("time", "<f8"), ("latitude", "<f8"), ("longitude", "<f8"), ("range_nm", "<f4"),
                      ("bearing_deg", "<f4"), ("ground_speed_kt", "<f4"), ("track_deg", "<f4"), ("altitude", "<i4"),
                      ("n_fixes", "<u4"), ("n_rejected", "<u4"), ("type_code", "u1"), ("flags", "u1"), ("cpr_odd", "u1"),
                      ("reserved8", "u1"), ("reserved", "<u4"), ("_pad", "<u4")])
FRAME_FIX_DTYPE = np.dtype([("latitude", "<f8"), ("longitude", "<f8"), ("range_nm", "<f4"), ("bearing_deg", "<f4"),
                            ("icao", "<u4"), ("flags", "<u4")])
assert SITE.itemsize == C.sizeof(AdsbSite) == 24 and FIX_DTYPE.itemsize == C.sizeof(AdsbFix) == 64
assert FRAME_FIX_DTYPE.itemsize == C.sizeof(AdsbFrameFix) == 32


ADSB_TRACK_MLAT_VALID = 0x1      # adsb_aircraft_mlat.flags / adsb_frame_mlat.flags: the record holds a fix
ADSB_TRACK_MLAT_ALTITUDE = 0x2   # that fix used the message's own altitude
ADSB_TRACK_MLAT_CHECKED = 0x4    # last_disagreement_m holds a value
ADSB_TRACK_MLAT_DISAGREE = 0x8   # adsb_frame_mlat.flags only: beyond the limit
ADSB_TRACK_MLAT_FAR = 0x10       # adsb_frame_mlat.flags only: the local decode was turned away


class AdsbAircraftMlat(C.Structure):
    """adsb_aircraft_mlat: an aircraft's newest multilaterated position and what its reported positions differ from the
    solved ones by, beside its record (tables with an mlat reserve)."""
    _fields_ = [("time", C.c_double), ("latitude", C.c_double), ("longitude", C.c_double), ("height_m", C.c_float),
                ("residual_rms_m", C.c_float), ("pdop", C.c_float), ("last_disagreement_m", C.c_float),
                ("max_disagreement_m", C.c_float), ("n_attempted", C.c_uint32), ("n_valid", C.c_uint32),
                ("n_checked", C.c_uint32), ("n_disagree", C.c_uint32), ("n_used", C.c_uint16), ("flags", C.c_uint8),
                ("reserved", C.c_uint8)]


class AdsbFrameMlat(C.Structure):
    _fields_ = [("disagreement_m", C.c_float), ("icao", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


AIRCRAFT_MLAT_DTYPE = np.dtype([("time", "<f8"), ("latitude", "<f8"), ("longitude", "<f8"), ("height_m", "<f4"),
                                ("residual_rms_m", "<f4"), ("pdop", "<f4"), ("last_disagreement_m", "<f4"),
                                ("max_disagreement_m", "<f4"), ("n_attempted", "<u4"), ("n_valid", "<u4"),
                                ("n_checked", "<u4"), ("n_disagree", "<u4"), ("n_used", "<u2"), ("flags", "u1"),
                                ("reserved", "u1")])
FRAME_MLAT_DTYPE = np.dtype([("disagreement_m", "<f4"), ("icao", "<u4"), ("flags", "<u4"), ("reserved", "<u4")])
assert AIRCRAFT_MLAT_DTYPE.itemsize == C.sizeof(AdsbAircraftMlat) == 64
assert FRAME_MLAT_DTYPE.itemsize == C.sizeof(AdsbFrameMlat) == 16


ADSB_TRACK_FILTER_RUNNING = 0x1     # adsb_aircraft_filter.flags: the record holds a state
ADSB_TRACK_FILTER_VELOCITY = 0x2    # run >= min_run: the velocities are worth showing
ADSB_TRACK_FILTER_HEIGHT = 0x4      # record: the up axis has been measured since the start; operand: it is
ADSB_TRACK_FILTER_USABLE = 0x100    # adsb_frame_filter.flags and adsb_filter_operand.flags
ADSB_TRACK_FILTER_APPLIED = 0x200   # adsb_frame_filter.flags only, as are the next four
ADSB_TRACK_FILTER_INIT = 0x400
ADSB_TRACK_FILTER_RESET = 0x800
ADSB_TRACK_FILTER_OUTLIER = 0x1000
ADSB_TRACK_FILTER_SKIPPED = 0x2000


class AdsbTrackFilterCfg(C.Structure):
    """adsb_track_filter_cfg: the policy of a filter reserve; 0 takes each default (96 bytes)."""
    _fields_ = [("accel_h", C.c_double), ("accel_v", C.c_double), ("range_sigma_m", C.c_double),
                ("altitude_sigma_m", C.c_double), ("gate", C.c_double), ("reset_gap_s", C.c_double),
                ("init_speed_sigma_h", C.c_double), ("init_speed_sigma_v", C.c_double), ("max_hdop", C.c_double),
                ("max_vdop", C.c_double), ("max_outliers", C.c_uint32), ("min_run", C.c_uint32),
                ("reserved", C.c_uint64)]


class AdsbAircraftFilter(C.Structure):
    """adsb_aircraft_filter: an aircraft's filtered mlat track, beside its record (tables with a filter reserve)."""
    _fields_ = [("time", C.c_double), ("latitude", C.c_double), ("longitude", C.c_double), ("height_m", C.c_double),
                ("v_north", C.c_double), ("v_east", C.c_double), ("v_up", C.c_double), ("p_north", C.c_double * 3),
                ("p_east", C.c_double * 3), ("p_up", C.c_double * 3), ("n_applied", C.c_uint32),
                ("n_outlier", C.c_uint32), ("n_reset", C.c_uint32), ("n_skipped", C.c_uint32), ("run", C.c_uint32),
                ("outliers_run", C.c_uint32), ("last_nis", C.c_float), ("flags", C.c_uint32),
                ("reserved", C.c_uint32 * 8)]


class AdsbFrameFilter(C.Structure):
    _fields_ = [("latitude", C.c_double), ("longitude", C.c_double), ("height_m", C.c_float), ("nis", C.c_float),
                ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class AdsbFilterOperand(C.Structure):
    _fields_ = [("time", C.c_double), ("latitude", C.c_double), ("longitude", C.c_double), ("rn", C.c_double),
                ("re", C.c_double), ("var_h", C.c_double), ("var_v", C.c_double), ("height_m", C.c_float),
                ("flags", C.c_uint32)]


AIRCRAFT_FILTER_DTYPE = np.dtype([("time", "<f8"), ("latitude", "<f8"), ("longitude", "<f8"), ("height_m", "<f8"),
                                  ("v_north", "<f8"), ("v_east", "<f8"), ("v_up", "<f8"), ("p_north", "<f8", (3,)),
                                  ("p_east", "<f8", (3,)), ("p_up", "<f8", (3,)), ("n_applied", "<u4"),
                                  ("n_outlier", "<u4"), ("n_reset", "<u4"), ("n_skipped", "<u4"), ("run", "<u4"),
                                  ("outliers_run", "<u4"), ("last_nis", "<f4"), ("flags", "<u4"),
                                  ("reserved", "<u4", (8,))])
FRAME_FILTER_DTYPE = np.dtype([("latitude", "<f8"), ("longitude", "<f8"), ("height_m", "<f4"), ("nis", "<f4"),
                               ("flags", "<u4"), ("reserved", "<u4")])
FILTER_OPERAND_DTYPE = np.dtype([("time", "<f8"), ("latitude", "<f8"), ("longitude", "<f8"), ("rn", "<f8"),
                                 ("re", "<f8"), ("var_h", "<f8"), ("var_v", "<f8"), ("height_m", "<f4"),
                                 ("flags", "<u4")])
assert AIRCRAFT_FILTER_DTYPE.itemsize == C.sizeof(AdsbAircraftFilter) == 192 and C.sizeof(AdsbTrackFilterCfg) == 96
assert FRAME_FILTER_DTYPE.itemsize == C.sizeof(AdsbFrameFilter) == 32
assert FILTER_OPERAND_DTYPE.itemsize == C.sizeof(AdsbFilterOperand) == 64


ADSB_TRACK_UNADDRESSED = 0x4        # point flag: the frame's address is not an aircraft's (update_modes)
ADSB_TRACK_MODES_ALT = 0x1          # adsb_aircraft_modes.flags: the ADSB_MODES_* bit values ...
ADSB_TRACK_MODES_SQUAWK = 0x4
ADSB_TRACK_MODES_GROUND = 0x8
ADSB_TRACK_MODES_ALERT = 0x10
ADSB_TRACK_MODES_SPI = 0x20
ADSB_TRACK_MODES_CALLSIGN = 0x40
ADSB_TRACK_MODES_STATUS = 0x100     # ... fs, ALERT and SPI hold a value
ADSB_TRACK_MODES_SQUITTER = 0x200   # the aircraft has sent an accepted DF17/18 frame


class AdsbAircraftModes(C.Structure):
    """adsb_aircraft_modes: what an aircraft's Mode S replies say, beside its record (tables with a modes reserve)."""
    _fields_ = [("altitude_time", C.c_double), ("squawk_time", C.c_double), ("callsign_time", C.c_double),
                ("altitude_ft", C.c_int32), ("squawk", C.c_uint16), ("flags", C.c_uint16), ("callsign", C.c_char * 8),
                ("n_replies", C.c_uint32), ("n_allcall", C.c_uint32), ("n_surveillance", C.c_uint32),
                ("n_airair", C.c_uint32), ("fs", C.c_uint8), ("last_df", C.c_uint8), ("reserved", C.c_uint8 * 6)]


AIRCRAFT_MODES_DTYPE = np.dtype([("altitude_time", "<f8"), ("squawk_time", "<f8"), ("callsign_time", "<f8"),
                                 ("altitude_ft", "<i4"), ("squawk", "<u2"), ("flags", "<u2"), ("callsign", "S8"),
                                 ("n_replies", "<u4"), ("n_allcall", "<u4"), ("n_surveillance", "<u4"),
                                 ("n_airair", "<u4"), ("fs", "u1"), ("last_df", "u1"), ("reserved", "u1", (6,))])
assert AIRCRAFT_MODES_DTYPE.itemsize == C.sizeof(AdsbAircraftModes) == 64

ADSB_COMMB_SETTLED = 5              # adsb_commb_rec.state, only in a table's per-frame output (update_commb)


class AdsbCommbSettleCfg(C.Structure):
    """adsb_commb_settle_cfg: the limits a table settles 5,0 against 6,0 with (16 bytes)."""
    _fields_ = [("max_age_s", C.c_double), ("max_speed_diff_kt", C.c_uint32), ("max_vrate_diff_fpm", C.c_uint32)]


class AdsbCommbBlock(C.Structure):
    """adsb_commb_block: the newest values of one register of an aircraft (32 bytes)."""
    _fields_ = [("time", C.c_double), ("value", C.c_int32 * 5), ("status", C.c_uint16), ("settled", C.c_uint16)]


class AdsbAircraftCommb(C.Structure):
    """adsb_aircraft_commb: what an aircraft's Comm-B replies say, beside its record (tables with a commb reserve)."""
    _fields_ = [("bds40", AdsbCommbBlock), ("bds50", AdsbCommbBlock), ("bds60", AdsbCommbBlock),
                ("n_commb", C.c_uint32), ("n_settled", C.c_uint32), ("n_ambiguous", C.c_uint32), ("n_none", C.c_uint32),
                ("capability", C.c_uint32), ("ra_word", C.c_uint32), ("ra_time", C.c_double)]


COMMB_BLOCK_DTYPE = np.dtype([("time", "<f8"), ("value", "<i4", (5,)), ("status", "<u2"), ("settled", "<u2")])
AIRCRAFT_COMMB_DTYPE = np.dtype([("bds40", COMMB_BLOCK_DTYPE), ("bds50", COMMB_BLOCK_DTYPE), ("bds60", COMMB_BLOCK_DTYPE),
                                 ("n_commb", "<u4"), ("n_settled", "<u4"), ("n_ambiguous", "<u4"), ("n_none", "<u4"),
                                 ("capability", "<u4"), ("ra_word", "<u4"), ("ra_time", "<f8")])
assert C.sizeof(AdsbCommbSettleCfg) == 16 and COMMB_BLOCK_DTYPE.itemsize == C.sizeof(AdsbCommbBlock) == 32
assert AIRCRAFT_COMMB_DTYPE.itemsize == C.sizeof(AdsbAircraftCommb) == 128

(ADSB_TRACK_ES_COUNTED, ADSB_TRACK_ES_POSITION, ADSB_TRACK_ES_VERSIONED, ADSB_TRACK_ES_STALE_A,
 ADSB_TRACK_ES_STALE_C) = 0x1, 0x2, 0x4, 0x8, 0x10                  # adsb_frame_integrity.flags


class AdsbEsTrackCfg(C.Structure):
    """adsb_es_track_cfg: how long a table uses a NIC supplement (16 bytes)."""
    _fields_ = [("max_age_s", C.c_double), ("reserved", C.c_uint32 * 2)]


class AdsbFrameIntegrity(C.Structure):
    """adsb_frame_integrity: NIC and Rc of one frame, resolved by a table with an es reserve (8 bytes)."""
    _fields_ = [("rc_dm", C.c_uint32), ("nic", C.c_uint8), ("version", C.c_uint8), ("supp", C.c_uint8), ("flags", C.c_uint8)]


class AdsbAircraftEs(C.Structure):
    """adsb_aircraft_es: what an aircraft's extended squitters say, beside its record (tables with an es reserve)."""
    _fields_ = ([(k, AdsbEsRec) for k in ("operational_airborne", "operational_surface", "target_state", "emergency", "acas_ra")]
                + [("time", C.c_double * 5)]
                + [(k, C.c_double) for k in ("version_time", "nic_a_time", "nic_c_time", "position_time")]
                + [("rc_dm", C.c_uint32)]
                + [(k, C.c_uint8) for k in ("nic", "position_tc", "nic_b", "position_supp", "version", "nic_a", "nic_c", "category")]
                + [("n_es", C.c_uint32), ("n_position", C.c_uint32)]
                + [(k, C.c_uint8) for k in ("nac_v", "velocity_flags", "has", "reserved")])


assert C.sizeof(AdsbEsTrackCfg) == 16 and C.sizeof(AdsbFrameIntegrity) == 8 and C.sizeof(AdsbAircraftEs) == 256


class AdsbTrackBankCfg(C.Structure):
    _fields_ = [("abi_version", C.c_uint32), ("n_receivers", C.c_uint32), ("max_aircraft", C.c_uint32),
                ("reserved", C.c_uint32), ("max_frames", C.c_uint64), ("seconds_per_sample", C.c_double)]


class AdsbPacketView(C.Structure):
    _fields_ = [("packet", C.c_uint8 * 14), ("downlink_format", C.c_uint8), ("capability", C.c_uint8),
                ("icao", C.c_uint32), ("msg_type", C.c_uint8), ("msg_kind", C.c_int32),
                ("callsign", C.c_char * 9), ("surveillance_status", C.c_uint8),
                ("nic_supplement", C.c_uint8), ("altitude", C.c_int32), ("cpr_time", C.c_uint8),
                ("cpr_odd", C.c_uint8), ("cpr_latitude", C.c_uint32), ("cpr_longitude", C.c_uint32),
                ("raw_msg", C.c_uint8 * 10)]


# name -> (restype, argtypes); every function include/*.h declares
_P = C.POINTER
PROTOTYPES = {
    "adsb_create": (C.c_int, [_P(AdsbCfg), _P(C.c_void_p)]),
    "adsb_destroy": (None, [C.c_void_p]),
    "adsb_strerror": (C.c_char_p, [C.c_int]),
    "adsb_demod": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, _P(AdsbFrame), C.c_size_t,
                             _P(C.c_size_t), _P(C.c_uint32)]),
    "adsb_demod_device_async": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_size_t, C.c_size_t]),
    "adsb_fetch": (C.c_int, [C.c_void_p, _P(AdsbFrame), C.c_size_t, _P(C.c_size_t), _P(C.c_uint64),
                             _P(C.c_uint64), _P(C.c_uint32)]),
    "adsb_fetch_counts": (C.c_int, [C.c_void_p, _P(C.c_uint64), _P(C.c_uint64), _P(C.c_uint32)]),
    "adsb_result_device": (C.c_int, [C.c_void_p, _P(C.c_void_p), _P(C.c_void_p)]),
    "adsb_decode_fields_device_async": (C.c_int, [C.c_void_p]),
    "adsb_fetch_fields": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, _P(C.c_size_t)]),
    "adsb_fields_device": (C.c_int, [C.c_void_p, _P(C.c_void_p)]),
    "adsb_levels_device_async": (C.c_int, [C.c_void_p]),
    "adsb_fetch_levels": (C.c_int, [C.c_void_p, _P(AdsbFrameLevel), C.c_size_t, _P(C.c_size_t)]),
    "adsb_levels_device": (C.c_int, [C.c_void_p, _P(C.c_void_p)]),
    "adsb_levels_of": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint64, C.c_void_p, C.c_size_t,
                                 _P(AdsbFrameLevel)]),
    "adsb_levels_modes_of": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_size_t, C.c_size_t, C.c_uint64, C.c_void_p,
                                       C.c_void_p, C.c_size_t, C.c_void_p]),
    "adsb_levels_modes_device": (C.c_int, [C.c_void_p, _P(C.c_void_p)]),
    "adsb_wire_device_async": (C.c_int, [C.c_void_p, _P(AdsbWireCfg)]),
    "adsb_fetch_wire": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, _P(C.c_size_t), C.c_void_p, C.c_size_t,
                                  _P(C.c_size_t)]),
    "adsb_wire_device": (C.c_int, [C.c_void_p, _P(C.c_void_p), _P(C.c_void_p), _P(C.c_void_p)]),
    "adsb_wire_of": (C.c_int, [C.c_void_p, _P(AdsbWireCfg), C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                               _P(C.c_size_t), C.c_void_p]),
    "adsb_debug_wire_geometry": (C.c_int, [_P(C.c_uint32), _P(C.c_uint32)]),
    "adsb_wire_in_of": (C.c_int, [C.c_void_p, _P(AdsbWireInCfg), C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32]),
    "adsb_fetch_wire_in": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, _P(C.c_size_t),
                                     C.c_void_p, C.c_void_p, C.c_uint32, _P(AdsbWireInHeader)]),
    "adsb_wire_in_device": (C.c_int, [C.c_void_p] + [_P(C.c_void_p)] * 6),
    "adsb_debug_wire_in_geometry": (C.c_int, [_P(C.c_uint32), _P(C.c_uint32)]),
    "adsb_modes_of": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t]),
    "adsb_fetch_modes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                   C.c_void_p, C.c_uint32, _P(AdsbModesHeader)]),
    "adsb_modes_device": (C.c_int, [C.c_void_p] + [_P(C.c_void_p)] * 5),
    "adsb_debug_modes_geometry": (C.c_int, [_P(C.c_uint32)]),
    "adsb_commb_of": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "adsb_fetch_commb": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, _P(AdsbCommbHeader)]),
    "adsb_commb_device": (C.c_int, [C.c_void_p, _P(C.c_void_p), _P(C.c_void_p)]),
    "adsb_debug_commb_geometry": (C.c_int, [_P(C.c_uint32)]),
    "adsb_es_of": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "adsb_fetch_es": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, _P(AdsbEsHeader)]),
    "adsb_es_device": (C.c_int, [C.c_void_p, _P(C.c_void_p), _P(C.c_void_p)]),
    "adsb_debug_es_geometry": (C.c_int, [_P(C.c_uint32)]),
    "adsb_replies_of": (C.c_int, [C.c_void_p, _P(AdsbRepliesCfg), C.c_void_p, C.c_uint32, C.c_size_t, C.c_size_t, C.c_void_p,
                                  C.c_size_t]),
    "adsb_fetch_replies": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, _P(C.c_size_t), C.c_void_p, _P(AdsbRepliesHeader)]),
    "adsb_replies_device": (C.c_int, [C.c_void_p] + [_P(C.c_void_p)] * 3),
    "adsb_debug_replies_geometry": (C.c_int, [_P(C.c_uint32), _P(C.c_uint32)]),
    "adsb_merge_lists_of": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p,
                                      C.c_void_p, C.c_void_p]),
    "adsb_correlate_launch": (C.c_int, [C.c_void_p, _P(AdsbCorrelateCfg), C.c_void_p]),
    "adsb_correlate_of": (C.c_int, [C.c_void_p, _P(AdsbCorrelateCfg), C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                    C.c_uint32, C.c_void_p]),
    "adsb_fetch_correlated": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, _P(C.c_size_t), C.c_void_p, C.c_size_t,
                                        _P(C.c_size_t)]),
    "adsb_correlated_device": (C.c_int, [C.c_void_p, _P(C.c_void_p), _P(C.c_void_p), _P(C.c_void_p), _P(C.c_void_p)]),
    "adsb_debug_correlate_geometry": (C.c_int, [_P(C.c_uint32)]),
    "adsb_multilaterate": (C.c_int, [C.c_void_p, _P(AdsbMlatCfg), C.c_void_p, C.c_uint32, C.c_void_p]),
    "adsb_multilaterate_of": (C.c_int, [C.c_void_p, _P(AdsbMlatCfg), C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t,
                                        C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]),
    "adsb_fetch_mlat": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, _P(C.c_size_t), _P(AdsbMlatHeader)]),
    "adsb_mlat_device": (C.c_int, [C.c_void_p, _P(C.c_void_p), _P(C.c_void_p)]),
    "adsb_debug_mlat_geometry": (C.c_int, [_P(C.c_uint32), _P(C.c_uint32)]),
    "adsb_clock_sync": (C.c_int, [C.c_void_p, _P(AdsbClockCfg), C.c_void_p, C.c_uint32, C.c_void_p]),
    "adsb_clock_sync_of": (C.c_int, [C.c_void_p, _P(AdsbClockCfg), C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t,
                                     C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]),
    "adsb_fetch_clocks": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, _P(C.c_size_t), _P(AdsbClockHeader)]),
    "adsb_clocks_device": (C.c_int, [C.c_void_p, _P(C.c_void_p), _P(C.c_void_p)]),
    "adsb_clock_apply": (C.c_int, [C.c_void_p]),
    "adsb_fetch_clock_receptions": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, _P(C.c_size_t), _P(C.c_size_t)]),
    "adsb_clock_receptions_device": (C.c_int, [C.c_void_p, _P(C.c_void_p), _P(C.c_size_t)]),
    "adsb_debug_clock_geometry": (C.c_int, [_P(C.c_uint32), _P(C.c_uint32)]),
    "adsb_track_device": (C.c_int, [C.c_void_p, C.c_double]),
    "adsb_fetch_track": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, _P(C.c_size_t), C.c_void_p, C.c_size_t,
                                   _P(C.c_size_t)]),
    "adsb_track_table_create": (C.c_int, [C.c_void_p, _P(AdsbTrackTableCfg), _P(C.c_void_p)]),
    "adsb_track_table_destroy": (None, [C.c_void_p]),
    "adsb_track_table_reset": (C.c_int, [C.c_void_p]),
    "adsb_track_table_update": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint64]),
    "adsb_track_table_fetch_points": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, _P(C.c_size_t)]),
    "adsb_track_table_fetch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, _P(C.c_size_t), _P(C.c_uint32)]),
    "adsb_track_table_expire": (C.c_int, [C.c_void_p, C.c_double]),
    "adsb_track_table_fetch_last_heard": (C.c_int, [C.c_void_p, _P(C.c_double), C.c_size_t, _P(C.c_size_t)]),
    "adsb_track_table_fetch_velocity": (C.c_int, [C.c_void_p, _P(AdsbVelocity), C.c_size_t, _P(C.c_size_t)]),
    "adsb_track_bank_create": (C.c_int, [C.c_void_p, _P(AdsbTrackBankCfg), _P(C.c_void_p)]),
    "adsb_track_bank_destroy": (None, [C.c_void_p]),
    "adsb_track_bank_reset": (C.c_int, [C.c_void_p]),
    "adsb_track_bank_update": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, _P(C.c_uint64), _P(C.c_uint64)]),
    "adsb_track_bank_update_launch": (C.c_int, [C.c_void_p, _P(C.c_uint64)]),
    "adsb_track_bank_fetch_points": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, _P(C.c_size_t)]),
    "adsb_track_bank_fetch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, _P(C.c_size_t), _P(C.c_uint64),
                                        _P(C.c_uint32)]),
    "adsb_track_bank_expire": (C.c_int, [C.c_void_p, _P(C.c_double)]),
    "adsb_track_bank_fetch_last_heard": (C.c_int, [C.c_void_p, _P(C.c_double), C.c_size_t, _P(C.c_size_t)]),
    "adsb_track_bank_fetch_velocity": (C.c_int, [C.c_void_p, _P(AdsbVelocity), C.c_size_t, _P(C.c_size_t)]),
    "adsb_track_bank_fuse_reserve": (C.c_int, [C.c_void_p, C.c_size_t]),
    "adsb_track_bank_fuse": (C.c_int, [C.c_void_p, C.c_double]),
    "adsb_track_bank_fetch_fused": (C.c_int, [C.c_void_p, _P(AdsbFusedAircraft), C.c_size_t, _P(C.c_size_t),
                                              _P(C.c_size_t), _P(C.c_uint32)]),
    "adsb_track_bank_fused_device": (C.c_int, [C.c_void_p, _P(C.c_void_p), _P(C.c_void_p)]),
    "adsb_track_table_summaries_reserve": (C.c_int, [C.c_void_p]),
    "adsb_track_table_fetch_summaries": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, _P(C.c_size_t)]),
    "adsb_track_table_summaries_device": (C.c_int, [C.c_void_p, _P(C.c_void_p)]),
    "adsb_track_table_fetch_changed": (C.c_int, [C.c_void_p, C.c_void_p, _P(C.c_double), _P(AdsbVelocity), C.c_size_t,
                                                 _P(C.c_size_t)]),
    "adsb_track_bank_summaries_reserve": (C.c_int, [C.c_void_p]),
    "adsb_track_bank_fetch_summaries": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, _P(C.c_size_t)]),
    "adsb_track_bank_summaries_device": (C.c_int, [C.c_void_p, _P(C.c_void_p)]),
    "adsb_track_bank_fetch_changed": (C.c_int, [C.c_void_p, C.c_void_p, _P(C.c_double), _P(AdsbVelocity), C.c_size_t,
                                                _P(C.c_size_t), _P(C.c_uint64)]),
    "adsb_track_table_levels_reserve": (C.c_int, [C.c_void_p]),
    "adsb_track_table_update_levels": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint64]),
    "adsb_track_table_fetch_levels": (C.c_int, [C.c_void_p, _P(AdsbAircraftLevel), C.c_size_t, _P(C.c_size_t)]),
    "adsb_track_table_levels_device": (C.c_int, [C.c_void_p, _P(C.c_void_p)]),
    "adsb_track_bank_levels_reserve": (C.c_int, [C.c_void_p]),
    "adsb_track_bank_levels_device": (C.c_int, [C.c_void_p, _P(C.c_void_p)]),
    "adsb_track_bank_update_levels": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, _P(C.c_uint64),
                                                _P(C.c_uint64)]),
    "adsb_track_bank_update_launch_levels": (C.c_int, [C.c_void_p, _P(C.c_uint64)]),
    "adsb_track_bank_fetch_levels": (C.c_int, [C.c_void_p, _P(AdsbAircraftLevel), C.c_size_t, _P(C.c_size_t)]),
    "adsb_track_bank_fetch_fused_levels": (C.c_int, [C.c_void_p, _P(AdsbFusedLevel), C.c_size_t, _P(C.c_size_t)]),
    "adsb_track_table_fixes_reserve": (C.c_int, [C.c_void_p, _P(AdsbSite)]),
    "adsb_track_table_fetch_fixes": (C.c_int, [C.c_void_p, _P(AdsbFix), C.c_size_t, _P(C.c_size_t)]),
    "adsb_track_table_fixes_device": (C.c_int, [C.c_void_p, _P(C.c_void_p)]),
    "adsb_track_table_fetch_frame_fixes": (C.c_int, [C.c_void_p, _P(AdsbFrameFix), C.c_size_t, _P(C.c_size_t)]),
    "adsb_track_table_mlat_reserve": (C.c_int, [C.c_void_p, C.c_double]),
    "adsb_track_table_update_mlat": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint64]),
    "adsb_track_table_fetch_mlat": (C.c_int, [C.c_void_p, _P(AdsbAircraftMlat), C.c_size_t, _P(C.c_size_t)]),
    "adsb_track_table_mlat_device": (C.c_int, [C.c_void_p, _P(C.c_void_p)]),
    "adsb_track_table_fetch_frame_mlat": (C.c_int, [C.c_void_p, _P(AdsbFrameMlat), C.c_size_t, _P(C.c_size_t)]),
    "adsb_track_table_filter_reserve": (C.c_int, [C.c_void_p, _P(AdsbTrackFilterCfg)]),
    "adsb_track_table_fetch_filter": (C.c_int, [C.c_void_p, _P(AdsbAircraftFilter), C.c_size_t, _P(C.c_size_t)]),
    "adsb_track_table_filter_device": (C.c_int, [C.c_void_p, _P(C.c_void_p)]),
    "adsb_track_table_fetch_frame_filter": (C.c_int, [C.c_void_p, _P(AdsbFrameFilter), C.c_size_t, _P(C.c_size_t)]),
    "adsb_debug_track_filter_operands": (C.c_int, [C.c_void_p, _P(AdsbFilterOperand), C.c_size_t, _P(C.c_size_t)]),
    "adsb_track_table_modes_reserve": (C.c_int, [C.c_void_p]),
    "adsb_track_table_update_modes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                                C.c_uint64]),
    "adsb_track_table_fetch_modes": (C.c_int, [C.c_void_p, _P(AdsbAircraftModes), C.c_size_t, _P(C.c_size_t)]),
    "adsb_track_table_modes_device": (C.c_int, [C.c_void_p, _P(C.c_void_p)]),
    "adsb_track_table_commb_reserve": (C.c_int, [C.c_void_p, _P(AdsbCommbSettleCfg)]),
    "adsb_track_table_update_commb": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.c_size_t, C.c_uint64]),
    "adsb_track_table_fetch_commb": (C.c_int, [C.c_void_p, _P(AdsbAircraftCommb), C.c_size_t, _P(C.c_size_t)]),
    "adsb_track_table_fetch_frame_commb": (C.c_int, [C.c_void_p, _P(AdsbCommbRec), C.c_size_t, _P(C.c_size_t)]),
    "adsb_track_table_commb_device": (C.c_int, [C.c_void_p, _P(C.c_void_p)]),
    "adsb_track_table_es_reserve": (C.c_int, [C.c_void_p, _P(AdsbEsTrackCfg)]),
    "adsb_track_table_update_es": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_size_t, C.c_uint64]),
    "adsb_track_table_fetch_es": (C.c_int, [C.c_void_p, _P(AdsbAircraftEs), C.c_size_t, _P(C.c_size_t)]),
    "adsb_track_table_fetch_frame_es": (C.c_int, [C.c_void_p, _P(AdsbFrameIntegrity), C.c_size_t, _P(C.c_size_t)]),
    "adsb_track_table_es_device": (C.c_int, [C.c_void_p, _P(C.c_void_p)]),
    "adsb_track_bank_fixes_reserve": (C.c_int, [C.c_void_p, _P(AdsbSite)]),
    "adsb_track_bank_fetch_fixes": (C.c_int, [C.c_void_p, _P(AdsbFix), C.c_size_t, _P(C.c_size_t)]),
    "adsb_track_bank_fixes_device": (C.c_int, [C.c_void_p, _P(C.c_void_p)]),
    "adsb_track_bank_fetch_frame_fixes": (C.c_int, [C.c_void_p, _P(AdsbFrameFix), C.c_size_t, _P(C.c_size_t)]),
    "adsb_cpr_num_zones": (C.c_uint32, [C.c_double]),
    "adsb_cpr_position": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, _P(C.c_double),
                                    _P(C.c_double)]),
    "adsb_tracker_create": (C.c_void_p, []),
    "adsb_tracker_destroy": (None, [C.c_void_p]),
    "adsb_tracker_update": (C.c_int, [C.c_void_p, C.c_void_p, C.c_double, _P(AdsbAircraftSummary)]),
    "adsb_tracker_count": (C.c_size_t, [C.c_void_p]),
    "adsb_tracker_get": (C.c_int, [C.c_void_p, C.c_uint32, _P(AdsbAircraftSummary)]),
    "adsb_stream": (C.c_void_p, [C.c_void_p]),
    "adsb_sample_type": (C.c_int, [C.c_void_p]),
    "adsb_stream_wait_results": (C.c_int, [C.c_void_p, C.c_void_p]),
    "adsb_feed_open": (C.c_int, [C.c_void_p, _P(AdsbFeedCfg), _P(C.c_void_p)]),
    "adsb_feed_acquire": (C.c_int, [C.c_void_p, _P(C.c_void_p)]),
    "adsb_feed_push": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "adsb_feed_pop": (C.c_int, [C.c_void_p, _P(AdsbFrame), C.c_size_t, _P(C.c_size_t), _P(C.c_uint32), _P(C.c_uint64)]),
    "adsb_feed_in_flight": (C.c_int, [C.c_void_p]),
    "adsb_feed_ready": (C.c_int, [C.c_void_p]),
    "adsb_feed_close": (None, [C.c_void_p]),
    "adsb_group_create": (C.c_int, [_P(AdsbGroupCfg), _P(C.c_void_p)]),
    "adsb_group_destroy": (None, [C.c_void_p]),
    "adsb_group_size": (C.c_uint32, [C.c_void_p]),
    "adsb_group_member": (C.c_void_p, [C.c_void_p, C.c_uint32]),
    "adsb_group_plan": (C.c_int, [C.c_uint64, C.c_uint32, _P(AdsbGroupShard)]),
    "adsb_group_demod": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, _P(AdsbFrame), C.c_size_t, _P(C.c_size_t),
                                   _P(C.c_uint32)]),
    "adsb_group_demod_host_async": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "adsb_group_demod_device_async": (C.c_int, [C.c_void_p, _P(C.c_void_p), C.c_size_t]),
    "adsb_group_fetch": (C.c_int, [C.c_void_p, _P(AdsbFrame), C.c_size_t, _P(C.c_size_t), _P(C.c_uint64), _P(C.c_uint32)]),
    "adsb_group_result_device": (C.c_int, [C.c_void_p, _P(C.c_void_p), _P(C.c_void_p)]),
    "adsb_set_result_target": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "adsb_set_stream_base": (C.c_int, [C.c_void_p, C.c_uint64]),
    "adsb_timing_enable": (C.c_int, [C.c_void_p, C.c_int]),
    "adsb_timing_read": (C.c_int, [C.c_void_p, _P(C.c_double), _P(C.c_double), _P(C.c_uint32)]),
    "adsb_timing_read3": (C.c_int, [C.c_void_p, _P(C.c_double), _P(C.c_double), _P(C.c_double), _P(C.c_uint32)]),
    "adsb_time_read_ceiling": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, _P(C.c_double)]),
    "adsb_debug_magnitudes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "adsb_debug_mag_mode": (C.c_int, [C.c_void_p]),
    "adsb_debug_fused_pass_only": (C.c_int, [C.c_void_p, C.c_int]),
    "adsb_debug_nsq_values": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "adsb_debug_scan": (C.c_int, [C.c_void_p]),
    "adsb_debug_code_table": (C.c_int, [C.c_void_p, C.c_void_p]),
    "adsb_measure_feed": (C.c_int, [C.c_int, C.c_int, C.c_size_t, C.c_double, _P(C.c_double), _P(C.c_double), _P(C.c_uint64)]),
    "adsb_measure_pinned_copy": (C.c_int, [C.c_int, C.c_size_t, C.c_int, _P(C.c_double)]),
    "adsb_debug_set_launch_index": (C.c_int, [C.c_void_p, C.c_uint32]),
    "adsb_debug_finish_stall": (C.c_int, [C.c_void_p, C.c_uint32]),
    "adsb_debug_pool_limit": (C.c_int, [C.c_void_p, C.c_int]),
    "adsb_debug_finish_geometry": (C.c_int, [_P(C.c_uint32), _P(C.c_uint32), _P(C.c_uint32), _P(C.c_uint32)]),
    "adsb_debug_tile_stamps": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, _P(C.c_size_t)]),
    "adsb_synth_default": (None, [_P(AdsbSynthCfg)]),
    "adsb_synth_fill_host": (C.c_int, [_P(AdsbSynthCfg), C.c_int, C.c_uint32, C.c_uint64, C.c_size_t,
                                       C.c_void_p]),
    "adsb_synth_fill_device": (C.c_int, [C.c_void_p, _P(AdsbSynthCfg), C.c_uint32, C.c_uint64,
                                         C.c_size_t, C.c_void_p]),
    "adsb_debug_synth_geometry": (C.c_int, [_P(C.c_uint32)]),
    "adsb_synth_slot": (C.c_int, [_P(AdsbSynthCfg), C.c_uint32, C.c_uint64, _P(C.c_uint64),
                                  _P(C.c_uint8 * 14), _P(C.c_uint8 * 14), _P(C.c_int)]),
    # include/adsb_host.h
    "adsb_packet_new": (C.c_int, [_P(C.c_uint8 * 14), _P(AdsbPacketView)]),
    "adsb_packet_new_from_string": (C.c_int, [C.c_char_p, _P(AdsbPacketView)]),
    "adsb_packet_display": (C.c_size_t, [_P(C.c_uint8 * 14), C.c_char_p, C.c_char_p, C.c_size_t]),
    "adsb_pipeline_playback": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_size_t,
                                         _P(AdsbFrame), C.c_size_t, _P(C.c_size_t), _P(C.c_uint64),
                                         C.c_char_p, C.c_size_t, _P(C.c_size_t)]),
    "adsb_pipeline_playback_carry": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_size_t,
                                               _P(AdsbFrame), C.c_size_t, _P(C.c_size_t), _P(C.c_uint64)]),
    "adsb_pipeline_run": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_size_t, C.c_uint32,
                                    _P(AdsbFrame), C.c_size_t, _P(C.c_size_t), _P(C.c_uint64),
                                    C.c_char_p, C.c_size_t, _P(C.c_size_t)]),
    "adsb_replay_file": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int, C.c_size_t, C.c_uint32, _P(AdsbFrame), C.c_size_t,
                                   _P(C.c_size_t), _P(C.c_uint64), _P(C.c_uint64), C.c_char_p, C.c_size_t, _P(C.c_size_t)]),
    "adsb_load_c16": (C.c_int, [C.c_char_p, _P(_P(C.c_int16)), _P(C.c_size_t)]),
    "adsb_save_c16": (C.c_int, [C.c_char_p, C.c_void_p, C.c_size_t]),
    "adsb_load_u8": (C.c_int, [C.c_char_p, _P(_P(C.c_int8)), _P(C.c_size_t)]),
    "adsb_free": (None, [C.c_void_p]),
    "adsb_host_frame_levels": (C.c_int, [C.c_int, C.c_void_p, C.c_size_t, C.c_uint64, C.c_void_p, C.c_size_t,
                                         _P(AdsbFrameLevel)]),
    "adsb_host_frame_levels_modes": (C.c_int, [C.c_int, C.c_void_p, C.c_uint32, C.c_size_t, C.c_size_t, C.c_uint64,
                                               C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "adsb_level_dbfs": (C.c_double, [C.c_int, C.c_uint64, C.c_uint32]),
    "adsb_host_wire_encode": (C.c_int, [_P(AdsbWireCfg), C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                        C.c_size_t, _P(C.c_size_t), C.c_void_p]),
    "adsb_host_wire_parse": (C.c_int, [_P(AdsbWireInCfg), C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_size_t, _P(C.c_size_t), C.c_void_p, C.c_void_p,
                                       _P(AdsbWireInHeader)]),
    "adsb_host_modes": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p,
                                  C.c_void_p, C.c_void_p, C.c_void_p, _P(AdsbModesHeader)]),
    "adsb_host_commb": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, _P(AdsbCommbHeader)]),
    "adsb_host_commb_as": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p]),
    "adsb_host_es": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, _P(AdsbEsHeader)]),
    "adsb_host_es_integrity": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, _P(C.c_uint32), _P(C.c_uint32)]),
    "adsb_host_replies": (C.c_int, [C.c_int, _P(AdsbRepliesCfg), C.c_void_p, C.c_uint32, C.c_size_t, C.c_size_t, C.c_void_p,
                                    C.c_size_t, C.c_void_p, C.c_size_t, _P(C.c_size_t), C.c_void_p, _P(AdsbRepliesHeader)]),
    "adsb_host_merge_lists": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p,
                                        C.c_void_p]),
    "adsb_host_correlate": (C.c_int, [_P(AdsbCorrelateCfg), C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint32,
                                      C.c_void_p, C.c_void_p, C.c_size_t, _P(C.c_size_t), C.c_void_p, C.c_void_p]),
    "adsb_host_multilaterate": (C.c_int, [_P(AdsbMlatCfg), C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p,
                                          C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, _P(AdsbMlatHeader)]),
    "adsb_host_clock_sync": (C.c_int, [_P(AdsbClockCfg), C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p,
                                       C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, _P(AdsbClockHeader), C.c_void_p]),
    "adsb_host_clock_apply": (C.c_int, [_P(AdsbClockCfg), C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t, C.c_void_p,
                                        C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]),
    "adsb_host_fix_of": (C.c_int, [_P(AdsbSite), _P(C.c_uint8 * 14), C.c_double, _P(AdsbFix), _P(C.c_uint32)]),
    "adsb_host_track_mlat_of": (C.c_int, [C.c_double, _P(C.c_uint8 * 14), _P(AdsbMlatFix), C.c_double,
                                          _P(AdsbAircraftMlat), _P(C.c_uint32), _P(C.c_float)]),
    "adsb_host_track_filter_operand": (C.c_int, [_P(AdsbTrackFilterCfg), _P(AdsbMlatFix), C.c_double, C.c_int,
                                                 _P(AdsbFilterOperand)]),
    "adsb_host_track_filter_step": (C.c_int, [_P(AdsbTrackFilterCfg), _P(AdsbAircraftFilter), _P(AdsbFilterOperand),
                                              _P(AdsbFrameFilter)]),
    "adsb_host_track_modes_of": (C.c_int, [C.c_void_p, C.c_double, _P(AdsbAircraftModes), _P(C.c_uint32)]),
    "adsb_host_track_modes_merge": (C.c_int, [_P(AdsbAircraftModes), _P(AdsbAircraftModes)]),
    "adsb_host_commb_settle": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, _P(AdsbCommbSettleCfg),
                                         C.c_void_p]),
    "adsb_host_commb_reference": (C.c_int, [C.c_void_p, C.c_double, C.c_void_p]),
    "adsb_host_track_commb_of": (C.c_int, [C.c_void_p, C.c_double, _P(AdsbAircraftCommb)]),
    "adsb_host_track_commb_merge": (C.c_int, [_P(AdsbAircraftCommb), _P(AdsbAircraftCommb)]),
    "adsb_host_es_resolve": (C.c_int, [C.c_void_p, C.c_double, C.c_void_p, _P(AdsbEsTrackCfg), C.c_void_p]),
    "adsb_host_track_es_of": (C.c_int, [C.c_void_p, C.c_void_p, C.c_double, C.c_void_p]),
    "adsb_host_track_es_merge": (C.c_int, [C.c_void_p, C.c_void_p]),
}

_lib = None


def _share_hip_runtime_with_torch():
    """One process must not hold two HIP runtimes: the second one to initialise finds no device.

    A PyTorch-ROCm wheel ships its own libamdhip64.so (SONAME libamdhip64.so.7, the same as /opt/rocm's) and
    loads it by file name, so `import torch` AFTER libadsb_hip.so has pulled in the system copy gives the process
    a second runtime ("No HIP GPUs are available"), while the other order is fine: the loader then binds
    libadsb_hip.so's NEEDED libamdhip64.so.7 to the copy that is already there.  When a torch wheel with a
    bundled runtime is installed, load that copy first, so that whichever of the two is imported first they
    share one runtime.  torch itself is not imported.  ADSB_HIP_SYSTEM_RUNTIME=1 opts out.
    """
    if os.environ.get("ADSB_HIP_SYSTEM_RUNTIME") == "1":
        return
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
        if spec is None or not spec.origin:
            return
        bundled = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
        if os.path.exists(bundled):
            C.CDLL(bundled, mode=C.RTLD_GLOBAL)
    except Exception:
        pass  # best effort: without it the import order decides, as before


def load():
    """Load the HIP library; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with ./build.sh (or __graft_entry__.build()). "
            "air_rs_amd has no CPU fallback for the demodulation path.")
    _share_hip_runtime_with_torch()
    lib = C.CDLL(LIB_PATH)
    lenient = os.environ.get("ADSB_HIP_LIB_LENIENT") == "1"  # A/B runs against libraries built from older sources
    for name, (res, args) in PROTOTYPES.items():
        if lenient and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def strerror(code):
    return load().adsb_strerror(int(code)).decode()


class AdsbError(RuntimeError):
    def __init__(self, code, where=""):
        self.code = int(code)
        super().__init__(f"{where}: {strerror(code)} (code {int(code)})")


def check(code, where=""):
    if code != ADSB_OK:
        raise AdsbError(code, where)
