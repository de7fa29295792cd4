"""air_rs_amd -- MI355X-native drop-in for air_rs's IQ -> packet thread (src/adsb.rs:92-122).

The product is the HIP library ``air_rs_amd/lib/libadsb_hip.so`` behind the C ABI in
``include/adsb_hip.h``; this package is the thin Python face used by the tests and bench.py.
"""
from ._lib import (ADSB_FIX_ALT, ADSB_FIX_REJECTED, ADSB_FIX_SPEED, ADSB_FIX_SURFACE, ADSB_FIX_TRACK, ADSB_FIX_VALID,
                   ADSB_LEVEL_VALID, ADSB_WIRE_AVR, ADSB_WIRE_AVR_MLAT, ADSB_WIRE_BEAST, ADSB_WIRE_MAX_BYTES, ADSB_WIRE_IN_CRC, ADSB_WIRE_IN_DF17, ADSB_FUSED_NONE, ADSB_TRACK_FUSED_TRUNCATED, ADSB_TRACK_NEW_POSITION, ADSB_TRACK_TABLE_FULL, ADSB_TRACK_UNTRACKED, ADSB_E_ARG, ADSB_E_CAPACITY,
                   ADSB_VELOCITY_DIRECTION, ADSB_VELOCITY_SPEED, ADSB_VELOCITY_VRATE,
                   ADSB_E_NODEVICE, ADSB_E_SHORT, ADSB_E_STATE,
                   ADSB_FLAG_INCOMPLETE, ADSB_FLAG_TRUNCATED, ADSB_OK, ADSB_SAMPLE_I8, ADSB_SAMPLE_I16, AdsbError, load,
                   ADSB_MLAT_C, ADSB_MLAT_MAX_RECEPTIONS, ADSB_MLAT_TIME_RECEPTION, ADSB_MLAT_TIME_TICKS,
                   ADSB_MLAT_USE_ALTITUDE, ADSB_MLAT_ATTEMPTED, ADSB_MLAT_CONVERGED, ADSB_MLAT_ALTITUDE, ADSB_MLAT_TOO_FEW,
                   ADSB_MLAT_TOO_MANY, ADSB_MLAT_SINGULAR, ADSB_MLAT_REJECTED_RESIDUAL, ADSB_MLAT_REJECTED_RANGE,
                   ADSB_MLAT_VALID, ADSB_MLAT_BAD_INDEX, ADSB_MLAT_HDR_BAD_INDEX,
                   ADSB_CLOCK_DRIFT, ADSB_CLOCK_REFERENCE, ADSB_CLOCK_REACHED, ADSB_CLOCK_HAS_DRIFT,
                   ADSB_CLOCK_HDR_BAD_INDEX, ADSB_CLOCK_HDR_DRIFT_DROPPED, ADSB_CLOCK_HDR_SINGULAR)
from .demod import (AIRCRAFT_DTYPE, AIRCRAFT_LEVEL_DTYPE, FUSED_LEVEL_DTYPE, FIELDS_DTYPE, FRAME_DTYPE, FUSED_DTYPE, LEVEL_DTYPE, LEVEL_PULSE_SAMPLES, LEVEL_QUIET_SAMPLES,
                    SITE, FIX_DTYPE, FRAME_FIX_DTYPE, host_fix_of,
                    host_frame_levels, host_wire_encode, host_wire_parse, WIRE_RX_DTYPE, WIRE_IN_HEADER_DTYPE, WireIn, host_correlate, frames_of_messages, MESSAGE_DTYPE, RECEPTION_DTYPE, level_dbfs, TRACK_POINT_DTYPE, VELOCITY_DTYPE, WINDOW, AdsbDemod, AdsbGroup, Feed, Tracker,
                    TrackBank, TrackTable,
                    MLAT_FIX_DTYPE, MLAT_RECEIVER_DTYPE, MLAT_HEADER_DTYPE, host_multilaterate,
                    CLOCK_DTYPE, CLOCK_HEADER_DTYPE, host_clock_sync, host_clock_apply,
                    group_plan,
                    cpr_position, packet_display, packet_new,
                    packet_new_from_string, synth_default, synth_fill_host, synth_slot, measure_feed, measure_pinned_copy)

__all__ = [
    "ADSB_OK", "ADSB_E_SHORT", "ADSB_E_ARG", "ADSB_E_CAPACITY", "ADSB_E_NODEVICE", "ADSB_E_STATE",
    "ADSB_FLAG_INCOMPLETE", "ADSB_FLAG_TRUNCATED", "ADSB_SAMPLE_I8", "ADSB_SAMPLE_I16", "AdsbError", "load", "FRAME_DTYPE",
    "FIELDS_DTYPE", "TRACK_POINT_DTYPE", "AIRCRAFT_DTYPE", "ADSB_TRACK_NEW_POSITION", "Tracker",
    "ADSB_TRACK_UNTRACKED", "ADSB_TRACK_TABLE_FULL", "TrackTable", "TrackBank", "cpr_position",
    "FUSED_DTYPE", "ADSB_FUSED_NONE", "ADSB_TRACK_FUSED_TRUNCATED", "AIRCRAFT_LEVEL_DTYPE", "FUSED_LEVEL_DTYPE",
    "VELOCITY_DTYPE", "ADSB_VELOCITY_SPEED", "ADSB_VELOCITY_DIRECTION", "ADSB_VELOCITY_VRATE",
    "WINDOW", "AdsbDemod", "AdsbGroup", "group_plan", "Feed", "packet_display", "packet_new", "packet_new_from_string",
    "LEVEL_DTYPE", "ADSB_LEVEL_VALID", "LEVEL_PULSE_SAMPLES", "LEVEL_QUIET_SAMPLES", "host_frame_levels", "level_dbfs",
    "SITE", "FIX_DTYPE", "FRAME_FIX_DTYPE", "host_fix_of", "ADSB_FIX_VALID", "ADSB_FIX_SURFACE", "ADSB_FIX_ALT",
    "ADSB_FIX_SPEED", "ADSB_FIX_TRACK", "ADSB_FIX_REJECTED",
    "ADSB_WIRE_BEAST", "ADSB_WIRE_AVR", "ADSB_WIRE_AVR_MLAT", "ADSB_WIRE_MAX_BYTES", "host_wire_encode",
    "ADSB_WIRE_IN_CRC", "ADSB_WIRE_IN_DF17", "host_wire_parse", "WIRE_RX_DTYPE", "WIRE_IN_HEADER_DTYPE", "WireIn",
    "MESSAGE_DTYPE", "RECEPTION_DTYPE", "host_correlate", "frames_of_messages",
    "MLAT_FIX_DTYPE", "MLAT_RECEIVER_DTYPE", "MLAT_HEADER_DTYPE", "host_multilaterate", "ADSB_MLAT_C",
    "ADSB_MLAT_MAX_RECEPTIONS", "ADSB_MLAT_TIME_RECEPTION", "ADSB_MLAT_TIME_TICKS", "ADSB_MLAT_USE_ALTITUDE",
    "ADSB_MLAT_ATTEMPTED", "ADSB_MLAT_CONVERGED", "ADSB_MLAT_ALTITUDE", "ADSB_MLAT_TOO_FEW", "ADSB_MLAT_TOO_MANY",
    "ADSB_MLAT_SINGULAR", "ADSB_MLAT_REJECTED_RESIDUAL", "ADSB_MLAT_REJECTED_RANGE", "ADSB_MLAT_VALID",
    "ADSB_MLAT_BAD_INDEX", "ADSB_MLAT_HDR_BAD_INDEX",
    "CLOCK_DTYPE", "CLOCK_HEADER_DTYPE", "host_clock_sync", "host_clock_apply", "ADSB_CLOCK_DRIFT", "ADSB_CLOCK_REFERENCE",
    "ADSB_CLOCK_REACHED", "ADSB_CLOCK_HAS_DRIFT", "ADSB_CLOCK_HDR_BAD_INDEX", "ADSB_CLOCK_HDR_DRIFT_DROPPED",
    "ADSB_CLOCK_HDR_SINGULAR",
    "synth_default", "synth_fill_host", "synth_slot", "measure_feed", "measure_pinned_copy",
]
