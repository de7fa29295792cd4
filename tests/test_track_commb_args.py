"""Comm-B registers per aircraft (adsb_track_table_*commb*, adsb_host_commb_settle, adsb_host_track_commb_*): the record
layouts, the declarations, and the argument checks that need no device (CPU tier).  The checks that need a table --
ADSB_E_STATE without a reserve, ADSB_E_CAPACITY, n = 0 -- are in tests/test_gpu_track_commb.py."""
import ctypes as C
import math
import os
import re

import numpy as np

from tests import track_commb_model as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("adsb_track_table_commb_reserve", "adsb_track_table_update_commb", "adsb_track_table_fetch_commb",
       "adsb_track_table_fetch_frame_commb", "adsb_track_table_commb_device")
HOST = ("adsb_host_commb_settle", "adsb_host_commb_reference", "adsb_host_track_commb_of", "adsb_host_track_commb_merge")


def test_record_sizes_and_offsets(lib):
    from air_rs_amd import _lib
    assert C.sizeof(_lib.AdsbCommbSettleCfg) == 16 and C.sizeof(_lib.AdsbCommbBlock) == 32
    assert C.sizeof(_lib.AdsbAircraftCommb) == 128 == lib.AIRCRAFT_COMMB_DTYPE.itemsize
    assert lib.AIRCRAFT_COMMB_DTYPE is _lib.AIRCRAFT_COMMB_DTYPE
    assert lib.AIRCRAFT_COMMB_DTYPE.names == T.MODEL_DTYPE.names
    for name, off in T.OFFSETS.items():
        assert getattr(_lib.AdsbAircraftCommb, name).offset == off == lib.AIRCRAFT_COMMB_DTYPE.fields[name][1], name
    for name, off in (("time", 0), ("value", 8), ("status", 28), ("settled", 30)):
        assert getattr(_lib.AdsbCommbBlock, name).offset == off == T.BLOCK_DTYPE.fields[name][1], name
    for name, off in (("max_age_s", 0), ("max_speed_diff_kt", 8), ("max_vrate_diff_fpm", 12)):
        assert getattr(_lib.AdsbCommbSettleCfg, name).offset == off, name
    assert lib.COMMB_SETTLED == 5 == T.SETTLED


def test_header_text():
    header = open(os.path.join(ROOT, "include", "adsb_hip.h")).read()
    assert "Comm-B registers per aircraft" in header
    assert re.search(r"#define\s+ADSB_ABI_VERSION\s+1u?\b", header)
    assert re.search(r"#define\s+ADSB_COMMB_SETTLED\s+5u\b", header)
    assert re.search(r"sizeof\(adsb_commb_settle_cfg\) == 16 && sizeof\(adsb_commb_block\) == 32 && "
                     r"sizeof\(adsb_aircraft_commb\) == 128", header)
    assert not re.search(r"adsb_track_bank_\w*commb", header)             # tables only


def test_declarations(lib):
    from air_rs_amd import _lib
    header = open(os.path.join(ROOT, "include", "adsb_hip.h")).read()
    host = open(os.path.join(ROOT, "include", "adsb_host.h")).read()
    L = _lib.load()
    for name in NEW:
        assert hasattr(L, name) and name in _lib.PROTOTYPES, name
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
    for name in HOST:
        assert hasattr(L, name) and name in _lib.PROTOTYPES and re.search(r"\bint\s+" + name + r"\s*\(", host), name
    for method in ("commb_reserve", "commb", "frame_commb", "commb_device"):
        assert callable(getattr(lib.TrackTable, method, None)), method
        assert not hasattr(lib.TrackBank, method), method
    sources = open(os.path.join(ROOT, "air_rs_amd", "csrc", "sources.list")).read().split()
    assert "host/adsb_track_commb.cpp" in sources
    for name in ("AIRCRAFT_COMMB_DTYPE", "COMMB_SETTLED", "aircraft_commb_physical", "host_commb_settle",
                 "host_commb_reference", "host_track_commb_of", "host_track_commb_merge"):
        assert name in lib.__all__, name


def test_bad_arguments(lib):
    from air_rs_amd import _lib
    L = _lib.load()
    fake = C.create_string_buffer(4096)                           # never dereferenced: every check below fails first
    h = C.addressof(fake)
    n, dev = C.c_size_t(), C.c_void_p()
    some = C.create_string_buffer(128)
    p = C.addressof(some)
    assert L.adsb_track_table_commb_reserve(None, None) == lib.ADSB_E_ARG
    for bad in (math.nan, -1.0, -math.inf):
        cfg = _lib.AdsbCommbSettleCfg(bad, 40, 1000)
        assert L.adsb_track_table_commb_reserve(h, C.byref(cfg)) == lib.ADSB_E_ARG
    assert L.adsb_track_table_update_commb(None, p, p, p, None, None, 1, 0) == lib.ADSB_E_ARG
    assert L.adsb_track_table_update_commb(None, None, None, None, None, None, 0, 0) == lib.ADSB_E_ARG
    assert L.adsb_track_table_update_commb(h, None, p, p, None, None, 1, 0) == lib.ADSB_E_ARG
    assert L.adsb_track_table_update_commb(h, p, None, p, None, None, 1, 0) == lib.ADSB_E_ARG
    assert L.adsb_track_table_update_commb(h, p, p, None, None, None, 1, 0) == lib.ADSB_E_ARG
    assert L.adsb_track_table_fetch_commb(None, None, 0, C.byref(n)) == lib.ADSB_E_ARG
    assert L.adsb_track_table_fetch_commb(h, None, 4, C.byref(n)) == lib.ADSB_E_ARG
    assert L.adsb_track_table_fetch_frame_commb(None, None, 0, C.byref(n)) == lib.ADSB_E_ARG
    assert L.adsb_track_table_fetch_frame_commb(h, None, 4, C.byref(n)) == lib.ADSB_E_ARG
    assert L.adsb_track_table_commb_device(None, C.byref(dev)) == lib.ADSB_E_ARG
    # the mirror
    assert L.adsb_host_commb_settle(None, p, None, 0.0, None, p) == lib.ADSB_E_ARG
    assert L.adsb_host_commb_settle(p, None, None, 0.0, None, p) == lib.ADSB_E_ARG
    assert L.adsb_host_commb_settle(p, p, None, 0.0, None, None) == lib.ADSB_E_ARG
    cfg = _lib.AdsbCommbSettleCfg(math.nan, 40, 1000)
    assert L.adsb_host_commb_settle(p, p, None, 0.0, C.byref(cfg), p) == lib.ADSB_E_ARG
    assert L.adsb_host_commb_settle(p, p, None, 0.0, None, p) == lib.ADSB_OK             # cfg NULL: the defaults
    assert L.adsb_host_commb_reference(None, 0.0, p) == L.adsb_host_commb_reference(p, 0.0, None) == lib.ADSB_E_ARG
    P = C.POINTER(_lib.AdsbAircraftCommb)
    one = _lib.AdsbAircraftCommb()
    assert L.adsb_host_track_commb_of(None, 0.0, C.byref(one)) == L.adsb_host_track_commb_of(p, 0.0, None) == lib.ADSB_E_ARG
    assert L.adsb_host_track_commb_merge(None, C.byref(one)) == L.adsb_host_track_commb_merge(C.byref(one), None) == lib.ADSB_E_ARG


def test_python_argument_checks_and_physical_units(lib):
    rec = np.zeros(2, dtype=lib.AIRCRAFT_COMMB_DTYPE)
    for b in ("bds40", "bds50", "bds60"):
        rec[b]["time"] = np.nan
    rec["ra_time"] = np.nan
    rec["bds50"][1] = (3.5, [-32, 1024, 430, 4, 360], 0x17, 1)        # the track rate's status bit is off
    rec["bds40"][1] = (2.0, [3008, 0, 10132, 0, 0], 0x05, 0)
    phys = lib.aircraft_commb_physical(rec)
    assert all(np.isnan(v[0]) for v in phys.values())
    assert phys["ground_speed_kt"][1] == 430 and phys["true_track_deg"][1] == 180.0 and phys["roll_deg"][1] == -5.625
    assert np.isnan(phys["track_rate_deg_s"][1]) and phys["true_airspeed_kt"][1] == 360
    assert phys["mcp_altitude_ft"][1] == 3008 and np.isnan(phys["fms_altitude_ft"][1])
    assert abs(phys["baro_setting_mb"][1] - 1013.2) < 1e-9 and np.isnan(phys["mach"][1])
    assert phys["bds50_settled"][1] == 1.0 and phys["bds40_settled"][1] == 0.0 and np.isnan(phys["bds60_settled"][1])
    assert phys["bds50_time"][1] == 3.5 and np.isnan(phys["bds60_time"][1])
