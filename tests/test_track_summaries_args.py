"""Per-frame summaries and the changed list of a track table / bank (adsb_track_{table,bank}_summaries_reserve,
_fetch_summaries, _summaries_device, _fetch_changed): every symbol is exported, declared in the header and in
_lib.PROTOTYPES, and rejects a NULL handle without touching its outputs; no device needed (CPU tier).  What needs a live
table (NULL arrays, ADSB_E_STATE, the results) is in tests/test_gpu_track_summaries.py."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("adsb_track_table_summaries_reserve", "adsb_track_table_fetch_summaries", "adsb_track_table_summaries_device",
       "adsb_track_table_fetch_changed", "adsb_track_bank_summaries_reserve", "adsb_track_bank_fetch_summaries",
       "adsb_track_bank_summaries_device", "adsb_track_bank_fetch_changed")


def test_summaries_symbols_are_exported_and_declared(lib):
    from air_rs_amd import _lib
    header = open(os.path.join(ROOT, "include", "adsb_hip.h")).read()
    L = _lib.load()
    for name in NEW:
        assert hasattr(L, name) and name in _lib.PROTOTYPES, name
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
    for cls in (lib.TrackTable, lib.TrackBank):
        for method in ("summaries_reserve", "summaries", "summaries_device", "changed"):
            assert callable(getattr(cls, method, None)), (cls.__name__, method)
    assert re.search(r"#define\s+ADSB_ABI_VERSION\s+1\b", header)          # the ABI version did not move


def test_summaries_record_is_the_48_byte_aircraft_record(lib):
    from air_rs_amd import _lib
    assert C.sizeof(_lib.AdsbAircraftRecord) == lib.AIRCRAFT_DTYPE.itemsize == 48


def test_summaries_null_handle_is_an_argument_error(lib):
    from air_rs_amd import _lib
    L = _lib.load()
    n = C.c_size_t(123)
    out = (_lib.AdsbAircraftRecord * 4)()
    heard = (C.c_double * 4)()
    vel = (_lib.AdsbVelocity * 4)()
    counts = (C.c_uint64 * 4)(7, 7, 7, 7)
    dev = C.c_void_p()
    for kind in ("table", "bank"):
        extra = (counts,) if kind == "bank" else ()
        assert getattr(L, f"adsb_track_{kind}_summaries_reserve")(None) == lib.ADSB_E_ARG
        fetch = getattr(L, f"adsb_track_{kind}_fetch_summaries")
        assert fetch(None, out, 4, C.byref(n)) == lib.ADSB_E_ARG
        assert fetch(None, None, 0, C.byref(n)) == lib.ADSB_E_ARG
        assert getattr(L, f"adsb_track_{kind}_summaries_device")(None, C.byref(dev)) == lib.ADSB_E_ARG
        changed = getattr(L, f"adsb_track_{kind}_fetch_changed")
        assert changed(None, out, heard, vel, 4, C.byref(n), *extra) == lib.ADSB_E_ARG
        assert changed(None, None, None, None, 0, C.byref(n), *((None,) if extra else ())) == lib.ADSB_E_ARG
    assert n.value == 123 and dev.value is None and list(counts) == [7, 7, 7, 7]   # untouched by a rejected call
