"""Correlate: the declarations, the structs' sizes and offsets, and the argument checks of every new entry point that
can be called without a device (CPU tier)."""
import ctypes as C
import os
import re

import numpy as np

from tests import correlate_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("adsb_correlate_launch", "adsb_correlate_of", "adsb_fetch_correlated", "adsb_correlated_device",
       "adsb_debug_correlate_geometry")
NEW_HOST = ("adsb_host_correlate",)
MESSAGE_LAYOUT = [("time", 0, 8), ("bytes", 8, 14), ("status", 22, 1), ("fixed_bit", 23, 1), ("first", 24, 4),
                  ("n_receptions", 28, 4), ("n_receivers", 32, 2), ("first_receiver", 34, 2), ("best_receiver", 36, 2),
                  ("reserved", 38, 2), ("n_clean", 40, 4), ("reserved2", 44, 4), ("span", 48, 8), ("best_signal_sum", 56, 8)]
RECEPTION_LAYOUT = [("time", 0, 8), ("frame", 8, 4), ("receiver", 12, 2), ("reserved", 14, 2)]


def _struct_fields(text, name):
    body = re.search(r"typedef\s+struct\s+" + name + r"\s*\{(.*?)\}\s*" + name + r"\s*;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", " ", body, flags=re.S)
    return [" ".join(d.split()) for d in body.split(";") if d.strip()]


def test_structs(lib):
    from air_rs_amd import _lib
    hip = open(os.path.join(ROOT, "include", "adsb_hip.h")).read()
    assert _struct_fields(hip, "adsb_correlate_cfg") == ["uint32_t window", "uint32_t use_levels", "uint64_t reserved"]
    assert C.sizeof(_lib.AdsbCorrelateCfg) == 16
    assert [f.split()[-1].split("[")[0] for f in _struct_fields(hip, "adsb_message")] == [n for n, _, _ in MESSAGE_LAYOUT]
    assert [f.split()[-1] for f in _struct_fields(hip, "adsb_reception")] == [n for n, _, _ in RECEPTION_LAYOUT]
    for ctype, dtypes, layout, size in ((_lib.AdsbMessage, (lib.MESSAGE_DTYPE, M.MESSAGE_DTYPE), MESSAGE_LAYOUT, 64),
                                        (_lib.AdsbReception, (lib.RECEPTION_DTYPE, M.RECEPTION_DTYPE), RECEPTION_LAYOUT, 16)):
        assert C.sizeof(ctype) == size
        assert [(n, getattr(ctype, n).offset, getattr(ctype, n).size) for n, _ in ctype._fields_] == layout
        for dt in dtypes:
            assert dt.itemsize == size
            assert [(n, dt.fields[n][1], dt.fields[n][0].itemsize) for n in dt.names] == layout
    assert re.search(r"#define\s+ADSB_ABI_VERSION\s+1\b", hip)                  # the feature only adds
    assert M.FRAME_DTYPE == lib.FRAME_DTYPE and M.LEVEL_DTYPE == lib.LEVEL_DTYPE


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
    for method in ("correlate", "correlate_async", "correlate_of", "correlate_of_async", "fetch_correlated",
                   "correlated_device"):
        assert callable(getattr(lib.AdsbDemod, method, None)), method
    assert callable(lib.host_correlate)
    sources = open(os.path.join(ROOT, "air_rs_amd", "csrc", "sources.list")).read().split()
    assert "adsb_correlate.hip" in sources and "host/adsb_correlate.cpp" in sources


def test_geometry(lib):
    from air_rs_amd import _lib
    L = _lib.load()
    b = C.c_uint32()
    assert L.adsb_debug_correlate_geometry(C.byref(b)) == lib.ADSB_OK
    assert b.value >= 64 and b.value % 64 == 0
    assert L.adsb_debug_correlate_geometry(None) == lib.ADSB_OK


def test_null_handles(lib):
    from air_rs_amd import _lib
    L = _lib.load()
    cfg = _lib.AdsbCorrelateCfg(10, 0, 0)
    fr, counts = M.build([[(0, bytes(14), 0, 0xFF)]])
    n, m = C.c_size_t(123), C.c_size_t(456)
    a, b, c, d = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    msgs = np.zeros(1, dtype=M.MESSAGE_DTYPE)
    recs = np.zeros(1, dtype=M.RECEPTION_DTYPE)
    assert L.adsb_correlate_launch(None, C.byref(cfg), None) == lib.ADSB_E_ARG
    assert L.adsb_correlate_launch(None, None, None) == lib.ADSB_E_ARG
    assert L.adsb_correlate_of(None, C.byref(cfg), fr.ctypes.data, None, 1, counts.ctypes.data, 1, None) == lib.ADSB_E_ARG
    assert L.adsb_correlate_of(None, None, None, None, 0, None, 0, None) == lib.ADSB_E_ARG
    assert L.adsb_fetch_correlated(None, msgs.ctypes.data, 1, C.byref(n), recs.ctypes.data, 1, C.byref(m)) == lib.ADSB_E_ARG
    assert L.adsb_correlated_device(None, C.byref(a), C.byref(b), C.byref(c), C.byref(d)) == lib.ADSB_E_ARG
    assert (n.value, m.value) == (123, 456) and not any(p.value for p in (a, b, c, d))
    assert not msgs.tobytes().strip(b"\0") and not recs.tobytes().strip(b"\0")


def test_host_correlate_bad_arguments(lib):
    from air_rs_amd import _lib
    L = _lib.load()
    fr, counts = M.build([[(5, bytes(14), 0, 0xFF), (9, bytes(14), 0, 0xFF)], [(6, bytes(14), 0, 0xFF)]])
    msgs = np.full(3, 0xEE, dtype=np.uint8).repeat(64).view(M.MESSAGE_DTYPE)
    fout = np.zeros(3, dtype=M.FRAME_DTYPE)
    recs = np.zeros(3, dtype=M.RECEPTION_DTYPE)
    n = C.c_size_t(123)
    good = _lib.AdsbCorrelateCfg(1, 0, 0)

    def call(cfg=C.byref(good), frames=fr.ctypes.data, count=3, cnt=counts, R=2, nm=C.byref(n), r=recs.ctypes.data):
        cnt = None if cnt is None else np.ascontiguousarray(cnt, dtype=np.uint64)
        return L.adsb_host_correlate(cfg, frames, None, count, None if cnt is None else cnt.ctypes.data, R, None,
                                     msgs.ctypes.data, 3, nm, fout.ctypes.data, r)

    assert call(cfg=None) == lib.ADSB_E_ARG
    assert call(frames=None) == lib.ADSB_E_ARG
    assert call(cnt=None) == lib.ADSB_E_ARG
    assert call(nm=None) == lib.ADSB_E_ARG
    assert call(r=None) == lib.ADSB_E_ARG
    assert call(R=0) == lib.ADSB_E_ARG
    assert call(cnt=[1] * 257, count=257, R=257) == lib.ADSB_E_ARG
    assert call(cnt=[2, 2]) == lib.ADSB_E_ARG and call(cnt=[1, 1]) == lib.ADSB_E_ARG      # counts do not sum to n
    assert call(cnt=[(1 << 64) - 1, 4]) == lib.ADSB_E_ARG                                # ... not even mod 2^64
    assert call(count=1 << 32, cnt=[1 << 32, 0]) == lib.ADSB_E_CAPACITY
    assert n.value == 123 and (msgs.view(np.uint8) == 0xEE).all() and not recs.tobytes().strip(b"\0")
    assert call() == lib.ADSB_OK and n.value == 2                                        # {5, 6} chain, 9 alone
    assert call(frames=None, count=0, cnt=[0, 0], r=None) == lib.ADSB_OK and n.value == 0
