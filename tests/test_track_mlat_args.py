"""Multilaterated positions per aircraft (adsb_track_table_*mlat*, adsb_host_track_mlat_of): the record layouts, the
declarations, and the argument checks that need no device (CPU tier).  The checks that need a table -- ADSB_E_STATE
without a reserve, ADSB_E_CAPACITY, n = 0 -- are in tests/test_gpu_track_mlat.py."""
import ctypes as C
import math
import os
import re

from tests import track_mlat_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("adsb_track_table_mlat_reserve", "adsb_track_table_update_mlat", "adsb_track_table_fetch_mlat",
       "adsb_track_table_mlat_device", "adsb_track_table_fetch_frame_mlat")
C_SIZE = {"double": 8, "float": 4, "uint32_t": 4, "uint16_t": 2, "uint8_t": 1}


def test_record_sizes_and_offsets(lib):
    from air_rs_amd import _lib
    assert C.sizeof(_lib.AdsbAircraftMlat) == 64 == lib.AIRCRAFT_MLAT_DTYPE.itemsize
    assert C.sizeof(_lib.AdsbFrameMlat) == 16 == lib.FRAME_MLAT_DTYPE.itemsize
    assert lib.AIRCRAFT_MLAT_DTYPE is _lib.AIRCRAFT_MLAT_DTYPE and lib.FRAME_MLAT_DTYPE is _lib.FRAME_MLAT_DTYPE
    for name, off in M.OFFSETS.items():
        assert getattr(_lib.AdsbAircraftMlat, name).offset == off == lib.AIRCRAFT_MLAT_DTYPE.fields[name][1], name
    for name in M.FRAME_DTYPE.names:
        assert getattr(_lib.AdsbFrameMlat, name).offset == M.FRAME_DTYPE.fields[name][1], name


def test_header_structs_flags_and_abi_version():
    """The header's two structs, laid out by the C rules from its own text; the ABI version is still 1."""
    header = open(os.path.join(ROOT, "include", "adsb_hip.h")).read()
    assert "Multilaterated positions per aircraft" in header
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

    assert fields("adsb_aircraft_mlat") == (M.OFFSETS, 64)
    assert fields("adsb_frame_mlat") == ({n: M.FRAME_DTYPE.fields[n][1] for n in M.FRAME_DTYPE.names}, 16)
    for name, value in (("VALID", M.VALID), ("ALTITUDE", M.ALTITUDE), ("CHECKED", M.CHECKED), ("DISAGREE", M.DISAGREE),
                        ("FAR", M.FAR)):
        assert int(re.search(r"#define\s+ADSB_TRACK_MLAT_" + name + r"\s+(0x[0-9a-fA-F]+)u", header).group(1), 16) == value
    assert not re.search(r"adsb_track_bank_\w*mlat", header)              # tables only


def test_declarations(lib):
    from air_rs_amd import _lib
    header = open(os.path.join(ROOT, "include", "adsb_hip.h")).read()
    host = open(os.path.join(ROOT, "include", "adsb_host.h")).read()
    L = _lib.load()
    for name in NEW:
        assert hasattr(L, name) and name in _lib.PROTOTYPES, name
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
    assert hasattr(L, "adsb_host_track_mlat_of") and re.search(r"\bint\s+adsb_host_track_mlat_of\s*\(", host)
    for method in ("mlat_reserve", "mlat", "frame_mlat", "mlat_device"):
        assert callable(getattr(lib.TrackTable, method, None)), method
        assert not hasattr(lib.TrackBank, method), method
    assert callable(lib.host_track_mlat_of)
    sources = open(os.path.join(ROOT, "air_rs_amd", "csrc", "sources.list")).read().split()
    assert "host/adsb_track_mlat.cpp" in sources
    assert (lib.ADSB_TRACK_MLAT_VALID, lib.ADSB_TRACK_MLAT_ALTITUDE, lib.ADSB_TRACK_MLAT_CHECKED,
            lib.ADSB_TRACK_MLAT_DISAGREE, lib.ADSB_TRACK_MLAT_FAR) == (1, 2, 4, 8, 16)


def test_bad_arguments(lib):
    from air_rs_amd import _lib
    L = _lib.load()
    fake = C.create_string_buffer(4096)                           # never dereferenced: every check below fails first
    h = C.addressof(fake)
    n, dev = C.c_size_t(), C.c_void_p()
    some = C.create_string_buffer(64)
    p = C.addressof(some)
    assert L.adsb_track_table_mlat_reserve(None, 1000.0) == lib.ADSB_E_ARG
    for bad in (0.0, -1.0, -0.0, math.nan, math.inf, -math.inf):
        assert L.adsb_track_table_mlat_reserve(h, bad) == lib.ADSB_E_ARG, bad
    assert L.adsb_track_table_update_mlat(None, p, p, None, 1, 0) == lib.ADSB_E_ARG
    assert L.adsb_track_table_update_mlat(None, None, None, None, 0, 0) == lib.ADSB_E_ARG
    assert L.adsb_track_table_update_mlat(h, None, p, None, 1, 0) == lib.ADSB_E_ARG
    assert L.adsb_track_table_update_mlat(h, p, None, None, 1, 0) == lib.ADSB_E_ARG
    assert L.adsb_track_table_update_mlat(h, None, None, p, 1, 0) == lib.ADSB_E_ARG
    assert L.adsb_track_table_fetch_mlat(None, None, 0, C.byref(n)) == lib.ADSB_E_ARG
    assert L.adsb_track_table_fetch_mlat(h, None, 4, C.byref(n)) == lib.ADSB_E_ARG
    assert L.adsb_track_table_fetch_frame_mlat(None, None, 0, C.byref(n)) == lib.ADSB_E_ARG
    assert L.adsb_track_table_fetch_frame_mlat(h, None, 4, C.byref(n)) == lib.ADSB_E_ARG
    assert L.adsb_track_table_mlat_device(None, C.byref(dev)) == lib.ADSB_E_ARG
