"""Positions from single messages (adsb_track_*_fixes_*, adsb_host_fix_of): the record layouts, the declarations, and
the argument checks that need no device (CPU tier).  The checks that need a store -- a bank's per-receiver sites and
ADSB_E_STATE on a store that holds aircraft -- are in tests/test_gpu_track_fixes.py."""
import ctypes as C
import math
import os
import re

from tests import fix_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("adsb_track_table_fixes_reserve", "adsb_track_table_fetch_fixes", "adsb_track_table_fixes_device",
       "adsb_track_table_fetch_frame_fixes", "adsb_track_bank_fixes_reserve", "adsb_track_bank_fetch_fixes",
       "adsb_track_bank_fixes_device", "adsb_track_bank_fetch_frame_fixes")
C_SIZE = {"double": 8, "float": 4, "int32_t": 4, "uint32_t": 4, "uint8_t": 1}
BAD_SITES = ((math.nan, 0.0, 100.0), (0.0, math.nan, 100.0), (0.0, 0.0, math.nan), (90.5, 0.0, 100.0),
             (-90.5, 0.0, 100.0), (0.0, 180.5, 100.0), (0.0, -180.5, 100.0), (0.0, 0.0, 0.0), (0.0, 0.0, -1.0),
             (0.0, 0.0, 180.5), (0.0, 0.0, math.inf))


def test_record_sizes_and_offsets(lib):
    from air_rs_amd import _lib
    assert C.sizeof(_lib.AdsbFix) == 64 == lib.FIX_DTYPE.itemsize
    assert C.sizeof(_lib.AdsbFrameFix) == 32 == lib.FRAME_FIX_DTYPE.itemsize
    assert C.sizeof(_lib.AdsbSite) == 24 == lib.SITE.itemsize
    assert lib.SITE is _lib.SITE and lib.FIX_DTYPE is _lib.FIX_DTYPE and lib.FRAME_FIX_DTYPE is _lib.FRAME_FIX_DTYPE
    for name, off in M.OFFSETS.items():
        assert getattr(_lib.AdsbFix, name).offset == off == lib.FIX_DTYPE.fields[name][1], name
    for name in M.FRAME_DTYPE.names:
        assert getattr(_lib.AdsbFrameFix, name).offset == M.FRAME_DTYPE.fields[name][1], name


def test_header_structs_and_abi_version():
    """The header's three structs, laid out by the C rules from its own text; the ABI version is still 1."""
    header = open(os.path.join(ROOT, "include", "adsb_hip.h")).read()
    assert re.search(r"#define\s+ADSB_ABI_VERSION\s+1u?\b", header)
    header = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)

    def fields(struct):
        body = re.search(r"typedef\s+struct\s+" + struct + r"\s*\{(.*?)\}\s*" + struct + r"\s*;", header, re.S).group(1)
        out, off, align = {}, 0, 1
        for decl in body.split(";"):
            decl = " ".join(decl.split())
            if not decl:
                continue
            ctype, names = decl.split(" ", 1)
            for item in names.split(","):
                size = C_SIZE[ctype]
                align = max(align, size)
                off = (off + size - 1) // size * size
                out[item.strip()] = off
                off += size
        return out, (off + align - 1) // align * align

    assert fields("adsb_fix") == (M.OFFSETS, 64)
    assert fields("adsb_frame_fix") == ({n: M.FRAME_DTYPE.fields[n][1] for n in M.FRAME_DTYPE.names}, 32)
    assert fields("adsb_site") == ({"latitude": 0, "longitude": 8, "max_range_nm": 16}, 24)
    for name, value in (("VALID", 1), ("SURFACE", 2), ("ALT", 4), ("SPEED", 8), ("TRACK", 16), ("REJECTED", 32)):
        assert int(re.search(r"#define\s+ADSB_FIX_" + name + r"\s+(0x[0-9a-fA-F]+)u", header).group(1), 16) == value


def test_declarations(lib):
    from air_rs_amd import _lib
    header = open(os.path.join(ROOT, "include", "adsb_hip.h")).read()
    host = open(os.path.join(ROOT, "include", "adsb_host.h")).read()
    L = _lib.load()
    for name in NEW:
        assert hasattr(L, name) and name in _lib.PROTOTYPES, name
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
    assert hasattr(L, "adsb_host_fix_of") and re.search(r"\bint\s+adsb_host_fix_of\s*\(", host)
    for cls in (lib.TrackTable, lib.TrackBank):
        for method in ("fixes_reserve", "fixes", "frame_fixes", "fixes_device"):
            assert callable(getattr(cls, method, None)), (cls, method)
    assert callable(lib.host_fix_of)


def test_bad_arguments(lib):
    from air_rs_amd import _lib
    L = _lib.load()
    fake = C.create_string_buffer(256)                            # never dereferenced: every check below fails first
    h = C.addressof(fake)
    n, dev = C.c_size_t(), C.c_void_p()
    good = _lib.AdsbSite(10.0, 20.0, 180.0)
    assert L.adsb_track_table_fixes_reserve(None, C.byref(good)) == lib.ADSB_E_ARG
    assert L.adsb_track_table_fixes_reserve(h, None) == lib.ADSB_E_ARG
    for bad in BAD_SITES:
        assert L.adsb_track_table_fixes_reserve(h, C.byref(_lib.AdsbSite(*bad))) == lib.ADSB_E_ARG, bad
    assert L.adsb_track_bank_fixes_reserve(None, C.byref(good)) == lib.ADSB_E_ARG
    assert L.adsb_track_bank_fixes_reserve(h, None) == lib.ADSB_E_ARG
    for prefix in ("adsb_track_table_", "adsb_track_bank_"):
        assert getattr(L, prefix + "fetch_fixes")(None, None, 0, C.byref(n)) == lib.ADSB_E_ARG
        assert getattr(L, prefix + "fetch_fixes")(h, None, 4, C.byref(n)) == lib.ADSB_E_ARG
        assert getattr(L, prefix + "fetch_frame_fixes")(None, None, 0, C.byref(n)) == lib.ADSB_E_ARG
        assert getattr(L, prefix + "fetch_frame_fixes")(h, None, 4, C.byref(n)) == lib.ADSB_E_ARG
        assert getattr(L, prefix + "fixes_device")(None, C.byref(dev)) == lib.ADSB_E_ARG


def test_model_merge_newest_wins_and_counts_saturate(oracle):
    """The model the GPU tests judge by, pinned by hand: newest accepted wins, a rejected or foreign frame leaves the fix,
    the counts saturate, and a cut changes nothing."""
    import numpy as np
    site = (40.0, -100.0, 180.0)
    icao = 0x4B1234
    items = [(100, M.frame_at(oracle, icao, site, 20.0, 10.0, 11, 0)),
             (200, M.frame_at(oracle, icao, site, 300.0, 10.0, 11, 1)),          # beyond half a zone: lands elsewhere
             (300, M.frame_at(oracle, icao, site, 181.0, 90.0, 11, 0)),          # rejected
             (300, M.frame_at(oracle, icao, site, 21.0, 10.0, 12, 1)),           # accepted: the newest
             (400, M.raw_frame(oracle, icao, 19 << 51 | 1 << 48)),               # velocity: nothing
             (500, M.frame_at(oracle, 0x4B0000, site, 5.0, 0.0, 6, 0, movement=39))]
    frames = np.zeros(len(items), dtype=[("offset", "<u8"), ("bytes", "u1", (14,))])
    for k, (off, b) in enumerate(items):
        frames[k]["offset"], frames[k]["bytes"] = off, np.frombuffer(b, dtype=np.uint8)
    st = M.apply({}, site, frames, sample_base=50, sps=0.5)
    a = st[icao]
    assert (a["type_code"], a["cpr_odd"], a["time"], a["n_rejected"]) == (12, 1, 175.0, 1) and a["n_fixes"] in (2, 3)
    assert abs(float(a["range_nm"]) - 21.0) < 0.01 and a["flags"] == M.VALID | M.ALT
    g = st[0x4B0000]
    assert g["flags"] == M.VALID | M.SURFACE | M.SPEED and g["ground_speed_kt"] == 15.0 and g["n_fixes"] == 1
    two = M.apply(M.apply({}, site, frames[:3], 50, 0.5), site, frames[3:], 50, 0.5)
    assert M.records(two, sorted(two)).tobytes() == M.records(st, sorted(st)).tobytes()
    rec = M.records(st, [1, icao])
    assert rec[0].tobytes() == M.empty().tobytes() and rec[0].tobytes()[8:] == bytes(56) and math.isnan(rec[0]["time"])
    full = a.copy()
    full["n_fixes"], full["n_rejected"] = M.U32, M.U32
    sat = M.apply({icao: full}, site, frames[2:4], 50, 0.5)[icao]
    assert sat["n_fixes"] == M.U32 and sat["n_rejected"] == M.U32
