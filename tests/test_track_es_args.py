"""Extended squitter status per aircraft (adsb_track_table_*es*, adsb_host_es_resolve, adsb_host_track_es_*): the record
layouts, the declarations, and the argument checks that need no device (CPU tier).  The checks that need a table --
ADSB_E_STATE without a reserve, ADSB_E_CAPACITY, n = 0 -- are in tests/test_gpu_track_es.py."""
import ctypes as C
import math
import os
import re

import numpy as np

from tests import track_es_model as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("adsb_track_table_es_reserve", "adsb_track_table_update_es", "adsb_track_table_fetch_es",
       "adsb_track_table_fetch_frame_es", "adsb_track_table_es_device")
HOST = ("adsb_host_es_resolve", "adsb_host_track_es_of", "adsb_host_track_es_merge")


def test_record_sizes_and_offsets(lib):
    from air_rs_amd import _lib
    assert C.sizeof(_lib.AdsbEsTrackCfg) == 16 and C.sizeof(_lib.AdsbFrameIntegrity) == 8
    assert C.sizeof(_lib.AdsbAircraftEs) == 256 == lib.AIRCRAFT_ES_DTYPE.itemsize
    assert lib.AIRCRAFT_ES_DTYPE.names == T.MODEL_DTYPE.names and lib.FRAME_INTEGRITY_DTYPE.names == T.FRAME_ES_DTYPE.names
    want = dict(operational_airborne=0, operational_surface=32, target_state=64, emergency=96, acas_ra=128, time=160,
                version_time=200, nic_a_time=208, nic_c_time=216, position_time=224, rc_dm=232, nic=236, position_tc=237,
                nic_b=238, position_supp=239, version=240, nic_a=241, nic_c=242, category=243, n_es=244, n_position=248,
                nac_v=252, velocity_flags=253, has=254, reserved=255)
    for name, off in want.items():
        assert getattr(_lib.AdsbAircraftEs, name).offset == off == lib.AIRCRAFT_ES_DTYPE.fields[name][1], name
        assert T.MODEL_DTYPE.fields[name][1] == off, name
    for name, off in (("rc_dm", 0), ("nic", 4), ("version", 5), ("supp", 6), ("flags", 7)):
        assert getattr(_lib.AdsbFrameIntegrity, name).offset == off == lib.FRAME_INTEGRITY_DTYPE.fields[name][1], name
    assert (lib.ADSB_TRACK_ES_COUNTED, lib.ADSB_TRACK_ES_POSITION, lib.ADSB_TRACK_ES_VERSIONED, lib.ADSB_TRACK_ES_STALE_A,
            lib.ADSB_TRACK_ES_STALE_C) == (T.COUNTED, T.POSITION, T.VERSIONED, T.STALE_A, T.STALE_C) == (1, 2, 4, 8, 16)


def test_header_text():
    header = open(os.path.join(ROOT, "include", "adsb_hip.h")).read()
    assert header.index("Comm-B registers per aircraft") < header.index("Extended squitter status per aircraft")
    assert re.search(r"#define\s+ADSB_ABI_VERSION\s+1u?\b", header)
    for name, value in (("COUNTED", "0x1u"), ("POSITION", "0x2u"), ("VERSIONED", "0x4u"), ("STALE_A", "0x8u"), ("STALE_C", "0x10u")):
        assert re.search(r"#define\s+ADSB_TRACK_ES_" + name + r"\s+" + value + r"\b", header), name
    assert re.search(r"sizeof\(adsb_es_track_cfg\) == 16 && sizeof\(adsb_frame_integrity\) == 8 &&\s+"
                     r"sizeof\(adsb_aircraft_es\) == 256", header)
    assert re.search(r"struct adsb_aircraft_es \{", header) and "typedef struct adsb_aircraft_es adsb_aircraft_es;" in header
    assert "policy, not a measurement" in header[header.index("Extended squitter status per aircraft"):]
    assert not re.search(r"adsb_track_bank_\w*_es\b", header)             # tables only


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
    for method in ("es_reserve", "es", "frame_es", "es_device"):
        assert callable(getattr(lib.TrackTable, method, None)), method
        assert not hasattr(lib.TrackBank, method), method
    sources = open(os.path.join(ROOT, "air_rs_amd", "csrc", "sources.list")).read().split()
    assert "host/adsb_track_es.cpp" in sources
    for name in ("AIRCRAFT_ES_DTYPE", "FRAME_INTEGRITY_DTYPE", "aircraft_es_physical", "host_es_resolve", "host_track_es_of",
                 "host_track_es_merge", "host_track_es", "AIRCRAFT_ES_COLUMNS", "aircraft_es_columns"):
        assert hasattr(lib, name) and name in lib.__all__, name


def test_null_arguments_without_a_device(lib):
    from air_rs_amd import _lib
    L = _lib.load()
    cfg = _lib.AdsbEsTrackCfg(60.0)
    n = C.c_size_t()
    buf = np.zeros(256, dtype=np.uint8)
    assert L.adsb_track_table_es_reserve(None, C.byref(cfg)) == lib.ADSB_E_ARG
    assert L.adsb_track_table_es_reserve(None, None) == lib.ADSB_E_ARG
    assert L.adsb_track_table_update_es(None, buf.ctypes.data, buf.ctypes.data, None, None, None, None, 1, 0) == lib.ADSB_E_ARG
    assert L.adsb_track_table_update_es(None, None, None, None, None, None, None, 0, 0) == lib.ADSB_E_ARG
    assert L.adsb_track_table_fetch_es(None, None, 0, C.byref(n)) == lib.ADSB_E_ARG
    assert L.adsb_track_table_fetch_frame_es(None, None, 0, C.byref(n)) == lib.ADSB_E_ARG
    assert L.adsb_track_table_es_device(None, None) == lib.ADSB_E_ARG


def test_host_arguments(lib):
    from air_rs_amd import _lib
    L = _lib.load()
    rec, out = np.zeros(1, dtype=lib.ES_DTYPE), np.zeros(1, dtype=lib.FRAME_INTEGRITY_DTYPE)
    one, other = np.zeros(1, dtype=lib.AIRCRAFT_ES_DTYPE), np.zeros(1, dtype=lib.AIRCRAFT_ES_DTYPE)
    ok = _lib.AdsbEsTrackCfg(60.0)
    assert L.adsb_host_es_resolve(rec.ctypes.data, 0.0, None, None, out.ctypes.data) == lib.ADSB_OK
    assert L.adsb_host_es_resolve(rec.ctypes.data, 0.0, one.ctypes.data, C.byref(ok), out.ctypes.data) == lib.ADSB_OK
    assert L.adsb_host_es_resolve(None, 0.0, None, None, out.ctypes.data) == lib.ADSB_E_ARG
    assert L.adsb_host_es_resolve(rec.ctypes.data, 0.0, None, None, None) == lib.ADSB_E_ARG
    for bad in (math.nan, -1.0, -math.inf):
        cfg = _lib.AdsbEsTrackCfg(bad)
        assert L.adsb_host_es_resolve(rec.ctypes.data, 0.0, None, C.byref(cfg), out.ctypes.data) == lib.ADSB_E_ARG, bad
    for fine in (0.0, math.inf):
        cfg = _lib.AdsbEsTrackCfg(fine)
        assert L.adsb_host_es_resolve(rec.ctypes.data, 0.0, None, C.byref(cfg), out.ctypes.data) == lib.ADSB_OK, fine
    assert L.adsb_host_track_es_of(rec.ctypes.data, out.ctypes.data, 0.0, one.ctypes.data) == lib.ADSB_OK
    for args in ((None, out.ctypes.data, one.ctypes.data), (rec.ctypes.data, None, one.ctypes.data), (rec.ctypes.data, out.ctypes.data, None)):
        assert L.adsb_host_track_es_of(args[0], args[1], 0.0, args[2]) == lib.ADSB_E_ARG
    assert L.adsb_host_track_es_merge(one.ctypes.data, other.ctypes.data) == lib.ADSB_OK
    assert L.adsb_host_track_es_merge(None, other.ctypes.data) == lib.ADSB_E_ARG
    assert L.adsb_host_track_es_merge(one.ctypes.data, None) == lib.ADSB_E_ARG


def test_python_argument_checks(lib):
    """update(es=) refuses lists of another length and commb without modes before any library call"""
    import pytest
    table = lib.TrackTable.__new__(lib.TrackTable)
    frames = np.zeros(3, dtype=lib.FRAME_DTYPE)
    with pytest.raises(ValueError):
        lib.TrackTable.update(table, frames, es=np.zeros(2, dtype=lib.ES_DTYPE))
    with pytest.raises(ValueError):
        lib.TrackTable.update(table, frames, es=np.zeros(3, dtype=lib.ES_DTYPE), commb=np.zeros(3, dtype=lib.COMMB_DTYPE))
    with pytest.raises(ValueError):
        lib.TrackTable.update_device(table, 1, 3, es_ptr=1, commb_ptr=1)
