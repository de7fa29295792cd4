"""Wire output: the declarations, the struct, and the argument checks of every new entry point that can be called without
a device (CPU tier)."""
import ctypes as C
import os
import re

import numpy as np

from tests import wire_model as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("adsb_wire_device_async", "adsb_fetch_wire", "adsb_wire_device", "adsb_wire_of", "adsb_debug_wire_geometry")
NEW_HOST = ("adsb_host_wire_encode",)


def test_struct_and_constants(lib):
    from air_rs_amd import _lib
    hip = open(os.path.join(ROOT, "include", "adsb_hip.h")).read()
    body = re.search(r"typedef\s+struct\s+adsb_wire_cfg\s*\{(.*?)\}\s*adsb_wire_cfg\s*;", hip, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", " ", body, flags=re.S)
    fields = [" ".join(d.split()) for d in body.split(";") if d.strip()]
    assert fields == ["uint32_t format", "uint32_t signal", "uint64_t tick_bias"]
    assert C.sizeof(_lib.AdsbWireCfg) == 4 + 4 + 8 == 16
    assert [(n, getattr(_lib.AdsbWireCfg, n).offset) for n, _ in _lib.AdsbWireCfg._fields_] == \
        [("format", 0), ("signal", 4), ("tick_bias", 8)]
    for name, val in (("ADSB_WIRE_BEAST", 0), ("ADSB_WIRE_AVR", 1), ("ADSB_WIRE_AVR_MLAT", 2), ("ADSB_WIRE_MAX_BYTES", 44)):
        assert re.search(r"#define\s+" + name + r"\s+" + str(val) + r"u?\b", hip), name
        assert getattr(lib, name) == getattr(_lib, name) == val
    assert W.FRAME_DTYPE == lib.FRAME_DTYPE and W.LEVEL_DTYPE == lib.LEVEL_DTYPE


def test_declarations(lib):
    from air_rs_amd import _lib
    L = _lib.load()
    hip = open(os.path.join(ROOT, "include", "adsb_hip.h")).read()
    host = open(os.path.join(ROOT, "include", "adsb_host.h")).read()
    for name in NEW:
        assert hasattr(L, name) and name in _lib.PROTOTYPES, name
        assert re.search(r"\bint\s+" + name + r"\s*\(", hip), name
    for name in NEW_HOST:
        assert hasattr(L, name) and name in _lib.PROTOTYPES, name
        assert re.search(r"\bint\s+" + name + r"\s*\(", host), name
    for method in ("wire", "wire_async", "fetch_wire", "wire_of", "wire_device"):
        assert callable(getattr(lib.AdsbDemod, method, None)), method
    assert callable(lib.host_wire_encode)
    assert "adsb_wire.hip" in open(os.path.join(ROOT, "air_rs_amd", "csrc", "sources.list")).read().split()


def test_geometry(lib):
    from air_rs_amd import _lib
    L = _lib.load()
    b, t = C.c_uint32(), C.c_uint32()
    assert L.adsb_debug_wire_geometry(C.byref(b), C.byref(t)) == lib.ADSB_OK
    assert b.value >= 64 and b.value % 64 == 0 and t.value >= 64
    assert L.adsb_debug_wire_geometry(None, None) == lib.ADSB_OK


def test_null_handles(lib):
    from air_rs_amd import _lib
    L = _lib.load()
    cfg = _lib.AdsbWireCfg(lib.ADSB_WIRE_BEAST, 1, 0)
    n, m = C.c_size_t(123), C.c_size_t(456)
    b, e, h = C.c_void_p(), C.c_void_p(), C.c_void_p()
    fr = W.frame_list([0], [W.KNOWN])
    out = np.zeros(64, dtype=np.uint8)
    ends = np.zeros(4, dtype=np.uint32)
    assert L.adsb_wire_device_async(None, C.byref(cfg)) == lib.ADSB_E_ARG
    assert L.adsb_wire_device_async(None, None) == lib.ADSB_E_ARG
    assert L.adsb_fetch_wire(None, out.ctypes.data, 64, C.byref(n), ends.ctypes.data, 4, C.byref(m)) == lib.ADSB_E_ARG
    assert L.adsb_fetch_wire(None, None, 0, C.byref(n), None, 0, C.byref(m)) == lib.ADSB_E_ARG
    assert L.adsb_wire_device(None, C.byref(b), C.byref(e), C.byref(h)) == lib.ADSB_E_ARG
    assert L.adsb_wire_of(None, C.byref(cfg), fr.ctypes.data, None, 1, out.ctypes.data, 64, C.byref(n),
                          ends.ctypes.data) == lib.ADSB_E_ARG
    assert L.adsb_wire_of(None, None, None, None, 0, None, 0, None, None) == lib.ADSB_E_ARG
    assert (n.value, m.value) == (123, 456) and b.value is None and e.value is None and h.value is None
    assert not out.any() and not ends.any()


def test_host_encode_bad_arguments(lib):
    from air_rs_amd import _lib
    L = _lib.load()
    fr = W.frame_list([0], [W.KNOWN])
    out = np.full(64, 0xEE, dtype=np.uint8)
    ends = np.full(1, 77, dtype=np.uint32)
    n = C.c_size_t(123)

    def call(cfg, st=lib.ADSB_SAMPLE_I8, frames=fr.ctypes.data, count=1, o=out.ctypes.data, cap=64, nb=C.byref(n)):
        return L.adsb_host_wire_encode(cfg, st, frames, None, count, o, cap, nb, ends.ctypes.data)

    good = _lib.AdsbWireCfg(lib.ADSB_WIRE_BEAST, 0, 0)
    assert call(None) == lib.ADSB_E_ARG
    assert call(C.byref(_lib.AdsbWireCfg(3, 0, 0))) == lib.ADSB_E_ARG                       # unknown format
    assert call(C.byref(_lib.AdsbWireCfg(0xFFFFFFFF, 0, 0))) == lib.ADSB_E_ARG
    assert call(C.byref(_lib.AdsbWireCfg(lib.ADSB_WIRE_AVR, 0, 1 << 48))) == lib.ADSB_E_ARG   # tick_bias >= 2^48
    assert call(C.byref(good), st=2) == lib.ADSB_E_ARG and call(C.byref(good), st=-1) == lib.ADSB_E_ARG
    assert call(C.byref(good), frames=None) == lib.ADSB_E_ARG
    assert call(C.byref(good), o=None) == lib.ADSB_E_ARG
    assert call(C.byref(good), nb=None) == lib.ADSB_E_ARG
    assert call(C.byref(good), frames=None, count=(1 << 32) // 44 + 1, o=None, cap=0) == lib.ADSB_E_ARG
    assert n.value == 123 and (out == 0xEE).all() and ends[0] == 77                         # untouched by rejected calls
    assert call(C.byref(_lib.AdsbWireCfg(lib.ADSB_WIRE_AVR_MLAT, 0, (1 << 48) - 1))) == lib.ADSB_OK and n.value == 43
    assert call(C.byref(good), frames=None, count=0, o=None, cap=0) == lib.ADSB_OK and n.value == 0
    # NULL ends and NULL out with cap 0: the length alone
    assert L.adsb_host_wire_encode(C.byref(good), lib.ADSB_SAMPLE_I8, fr.ctypes.data, None, 1, None, 0, C.byref(n),
                                   None) == lib.ADSB_OK and n.value == 23
