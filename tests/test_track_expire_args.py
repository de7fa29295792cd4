"""Expiry of the track table and bank (adsb_track_*_expire, adsb_track_*_fetch_last_heard): the entry points are
exported and declared, and reject bad arguments before touching a device (CPU tier: no GPU is needed for any of
these)."""
import ctypes as C
import math
import os
import re

from air_rs_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("adsb_track_table_expire", "adsb_track_bank_expire", "adsb_track_table_fetch_last_heard",
       "adsb_track_bank_fetch_last_heard")


def test_expire_symbols_are_exported_and_declared(lib):
    L = _lib.load()
    header = open(os.path.join(ROOT, "include", "adsb_hip.h")).read()
    for name in NEW:
        assert hasattr(L, name), name                             # exported by libadsb_hip.so
        assert name in _lib.PROTOTYPES, name
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
    assert _lib.PROTOTYPES["adsb_track_table_expire"][1][1] is C.c_double
    assert "never evicted" not in header


def test_expire_bad_arguments(lib):
    L = _lib.load()
    fake = C.create_string_buffer(64)                             # never dereferenced: every check below fails first
    n = C.c_size_t(123)
    before = (C.c_double * 4)(0.0, 1.0, 2.0, 3.0)
    out = (C.c_double * 4)()
    assert L.adsb_track_table_expire(None, 1.0) == lib.ADSB_E_ARG
    assert L.adsb_track_table_expire(None, -math.inf) == lib.ADSB_E_ARG
    assert L.adsb_track_table_expire(C.addressof(fake), math.nan) == lib.ADSB_E_ARG
    assert L.adsb_track_bank_expire(None, before) == lib.ADSB_E_ARG
    assert L.adsb_track_bank_expire(C.addressof(fake), None) == lib.ADSB_E_ARG
    assert L.adsb_track_table_fetch_last_heard(None, out, 4, C.byref(n)) == lib.ADSB_E_ARG
    assert L.adsb_track_table_fetch_last_heard(C.addressof(fake), None, 4, C.byref(n)) == lib.ADSB_E_ARG
    assert L.adsb_track_bank_fetch_last_heard(None, out, 4, C.byref(n)) == lib.ADSB_E_ARG
    assert L.adsb_track_bank_fetch_last_heard(C.addressof(fake), None, 4, C.byref(n)) == lib.ADSB_E_ARG
    assert n.value == 123                                         # untouched by a rejected call


def test_expire_python_methods(lib):
    for cls in (lib.TrackTable, lib.TrackBank):
        assert callable(getattr(cls, "expire", None)) and callable(getattr(cls, "last_heard", None)), cls
