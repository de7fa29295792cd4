"""Multilaterate: the declarations, the structs' sizes and offsets, the constants, and every argument check that can be
reached without a device (CPU tier)."""
import ctypes as C
import math
import os
import re

import numpy as np

from tests import mlat_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("adsb_multilaterate", "adsb_multilaterate_of", "adsb_fetch_mlat", "adsb_mlat_device", "adsb_debug_mlat_geometry")
FIX_LAYOUT = [("latitude", 0, 8), ("longitude", 8, 8), ("height_m", 16, 8), ("time_s", 24, 8), ("residual_rms_m", 32, 4),
              ("pdop", 36, 4), ("hdop", 40, 4), ("vdop", 44, 4), ("n_used", 48, 2), ("iterations", 50, 2), ("flags", 52, 4),
              ("reserved", 56, 8)]
RECEIVER_LAYOUT = [("latitude", 0, 8), ("longitude", 8, 8), ("height_m", 16, 8), ("clock_offset_s", 24, 8)]


def test_structs_and_constants(lib):
    from air_rs_amd import _lib
    hip = open(os.path.join(ROOT, "include", "adsb_hip.h")).read()
    for ctype, dtypes, layout, size in ((_lib.AdsbMlatFix, (lib.MLAT_FIX_DTYPE, M.FIX_DTYPE), FIX_LAYOUT, 64),
                                        (_lib.AdsbMlatReceiver, (lib.MLAT_RECEIVER_DTYPE, M.RECEIVER_DTYPE),
                                         RECEIVER_LAYOUT, 32)):
        assert C.sizeof(ctype) == size
        assert [(n, getattr(ctype, n).offset, getattr(ctype, n).size) for n, _ in ctype._fields_] == layout
        for dt in dtypes:
            assert dt.itemsize == size
            assert [(n, dt.fields[n][1], dt.fields[n][0].itemsize) for n in dt.names] == layout
    assert C.sizeof(_lib.AdsbMlatCfg) == 64 and C.sizeof(_lib.AdsbMlatHeader) == 32 == lib.MLAT_HEADER_DTYPE.itemsize
    for name, want in (("ATTEMPTED", M.ATTEMPTED), ("CONVERGED", M.CONVERGED), ("ALTITUDE", M.ALTITUDE),
                       ("TOO_FEW", M.TOO_FEW), ("TOO_MANY", M.TOO_MANY), ("SINGULAR", M.SINGULAR),
                       ("REJECTED_RESIDUAL", M.REJECTED_RESIDUAL), ("REJECTED_RANGE", M.REJECTED_RANGE),
                       ("VALID", M.VALID), ("BAD_INDEX", M.BAD_INDEX), ("MAX_RECEPTIONS", 256), ("TIME_RECEPTION", 0),
                       ("TIME_TICKS", 1), ("USE_ALTITUDE", 1)):
        got = re.search(r"#define\s+ADSB_MLAT_" + name + r"\s+(\w+)", hip).group(1)
        assert int(got.rstrip("u"), 0) == want == getattr(lib, "ADSB_MLAT_" + name), name
    assert re.search(r"#define\s+ADSB_MLAT_C\s+\(299792458\.0 / 1\.0003\)", hip)
    assert lib.ADSB_MLAT_C == M.C_AIR == 299792458.0 / 1.0003
    assert re.search(r"#define\s+ADSB_ABI_VERSION\s+1\b", hip)                  # the feature only adds


def test_declarations(lib):
    from air_rs_amd import _lib
    L = _lib.load()
    hip = open(os.path.join(ROOT, "include", "adsb_hip.h")).read()
    host = open(os.path.join(ROOT, "include", "adsb_host.h")).read()
    for name in NEW:
        assert hasattr(L, name) and name in _lib.PROTOTYPES, name
        assert re.search(r"\bint\s+" + name + r"\s*\(", hip), name
    assert hasattr(L, "adsb_host_multilaterate") and re.search(r"\bint\s+adsb_host_multilaterate\s*\(", host)
    for method in ("multilaterate", "multilaterate_async", "multilaterate_of", "multilaterate_of_async", "fetch_mlat",
                   "mlat_device"):
        assert callable(getattr(lib.AdsbDemod, method, None)), method
    assert callable(lib.host_multilaterate)
    sources = open(os.path.join(ROOT, "air_rs_amd", "csrc", "sources.list")).read().split()
    assert {"adsb_mlat.hip", "adsb_mlat_api.cpp", "host/adsb_mlat.cpp"} <= set(sources)


def test_geometry(lib):
    from air_rs_amd import _lib
    L = _lib.load()
    lanes, per = C.c_uint32(), C.c_uint32()
    assert L.adsb_debug_mlat_geometry(C.byref(lanes), C.byref(per)) == lib.ADSB_OK
    assert lanes.value == 16 and per.value * lanes.value == 256
    assert L.adsb_debug_mlat_geometry(None, None) == lib.ADSB_OK


def _one_message():
    msgs = np.zeros(1, dtype=M.MESSAGE_DTYPE)
    recs = np.zeros(4, dtype=M.RECEPTION_DTYPE)
    msgs["n_receptions"], recs["receiver"], recs["frame"] = 4, [0, 1, 2, 3], [0, 1, 2, 3]
    recs["time"] = [100, 140, 90_000, 100_000]
    rcv = np.zeros(4, dtype=M.RECEIVER_DTYPE)
    rcv["latitude"], rcv["longitude"], rcv["height_m"] = [47.0, 47.5, 47.9, 47.4], [8.0, 9.1, 8.3, 8.9], [400, 900, 1500, 600]
    return msgs, recs, rcv


def test_null_handles(lib):
    from air_rs_amd import _lib
    L = _lib.load()
    msgs, recs, rcv = _one_message()
    cfg = _lib.AdsbMlatCfg(0, 0, 0, 0, 1e-9, 0, 0, 0, 0, 0)
    fixes = np.zeros(1, dtype=M.FIX_DTYPE)
    n, a, b = C.c_size_t(123), C.c_void_p(), C.c_void_p()
    hdr = _lib.AdsbMlatHeader(7, 7, 7, 7)
    assert L.adsb_multilaterate(None, C.byref(cfg), rcv.ctypes.data, 4, None) == lib.ADSB_E_ARG
    assert L.adsb_multilaterate_of(None, C.byref(cfg), rcv.ctypes.data, 4, msgs.ctypes.data, 1, recs.ctypes.data, 4,
                                   None, 0) == lib.ADSB_E_ARG
    assert L.adsb_fetch_mlat(None, fixes.ctypes.data, 1, C.byref(n), C.byref(hdr)) == lib.ADSB_E_ARG
    assert L.adsb_mlat_device(None, C.byref(a), C.byref(b)) == lib.ADSB_E_ARG
    assert n.value == 123 and hdr.n_messages == 7 and not a.value and not b.value and not fixes.tobytes().strip(b"\0")


def test_host_multilaterate_bad_arguments(lib):
    from air_rs_amd import _lib
    L = _lib.load()
    msgs, recs, rcv = _one_message()
    rx = np.zeros(4, dtype=M.WIRE_RX_DTYPE)
    fixes = np.full(64, 0xEE, dtype=np.uint8).view(M.FIX_DTYPE)
    hdr = _lib.AdsbMlatHeader(7, 7, 7, 7)

    def cfg(time_source=0, flags=0, min_receivers=0, max_iterations=0, spt=1e-9, tol=0.0, res=0.0, rng=0.0, alt=0.0):
        return _lib.AdsbMlatCfg(time_source, flags, min_receivers, max_iterations, spt, tol, res, rng, alt, 0)

    def call(c=None, r=rcv, R=4, m=msgs, nm=1, rc=recs, nr=4, x=None, nx=0, f=fixes, no_cfg=False):
        c = c or cfg()
        ptr = lambda v: None if v is None else v.ctypes.data
        return L.adsb_host_multilaterate(None if no_cfg else C.byref(c), ptr(r), R, ptr(m), nm, ptr(rc), nr, ptr(x), nx,
                                         ptr(f), C.byref(hdr))

    E = lib.ADSB_E_ARG
    assert call(no_cfg=True) == E and call(r=None) == E and call(m=None) == E and call(rc=None) == E and call(f=None) == E
    assert call(R=0) == E and call(R=257) == E
    assert call(c=cfg(time_source=2)) == E and call(c=cfg(flags=2)) == E
    assert call(c=cfg(min_receivers=257)) == E and call(c=cfg(max_iterations=1001)) == E
    assert call(c=cfg(spt=0.0)) == E                                        # RECEPTION needs a tick length
    for bad in (math.nan, math.inf, -1.0):
        assert call(c=cfg(spt=bad)) == E and call(c=cfg(tol=bad)) == E and call(c=cfg(res=bad)) == E
        assert call(c=cfg(rng=bad)) == E
    assert call(c=cfg(alt=math.nan)) == E and call(c=cfg(alt=1e6)) == E
    assert call(c=cfg(time_source=1)) == E                                  # TICKS without rx
    for field, bad in (("latitude", 90.5), ("latitude", math.nan), ("longitude", -181.0), ("height_m", math.inf),
                       ("height_m", 2e5), ("clock_offset_s", math.nan), ("clock_offset_s", 1e7)):
        r2 = rcv.copy()
        r2[field][2] = bad
        assert call(r=r2) == E, (field, bad)
    assert call(nm=1 << 32) == lib.ADSB_E_CAPACITY and call(nr=1 << 32) == lib.ADSB_E_CAPACITY
    assert hdr.n_messages == 7 and (fixes.view(np.uint8) == 0xEE).all()     # nothing was written by a refused call

    assert call() == lib.ADSB_OK and hdr.n_messages == 1 and fixes["flags"][0] & M.ATTEMPTED
    assert call(c=cfg(time_source=1, spt=0.0), x=rx, nx=4) == lib.ADSB_OK   # TICKS: 0 takes 1 / 12e6
    # indices the lists do not have: reported, never read
    assert call(R=3) == E and fixes["flags"][0] == M.BAD_INDEX and hdr.flags == 1          # receiver 3 of 3
    assert call(nr=3) == E and fixes["flags"][0] == M.BAD_INDEX                             # receptions past recs[]
    assert call(c=cfg(time_source=1), x=rx, nx=3) == E and fixes["flags"][0] == M.BAD_INDEX  # frame 3 of 3
    assert fixes[0].tobytes()[:52] == bytes(52)
    assert call(m=None, nm=0, rc=None, nr=0, f=None) == lib.ADSB_OK and hdr.n_messages == 0
