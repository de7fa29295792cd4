"""Mode S replies per aircraft (adsb_track_table_*modes*, adsb_host_track_modes_*): the record layout, the declarations,
and the argument checks that need no device (CPU tier).  The checks that need a table -- ADSB_E_STATE without a reserve,
ADSB_E_CAPACITY, n = 0 -- are in tests/test_gpu_track_modes.py."""
import ctypes as C
import os
import re

from tests import track_modes_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("adsb_track_table_modes_reserve", "adsb_track_table_update_modes", "adsb_track_table_fetch_modes",
       "adsb_track_table_modes_device")
HOST = ("adsb_host_track_modes_of", "adsb_host_track_modes_merge")
C_SIZE = {"double": 8, "float": 4, "uint32_t": 4, "int32_t": 4, "uint16_t": 2, "uint8_t": 1, "char": 1}


def test_record_size_and_offsets(lib):
    from air_rs_amd import _lib
    assert C.sizeof(_lib.AdsbAircraftModes) == 64 == lib.AIRCRAFT_MODES_DTYPE.itemsize
    assert lib.AIRCRAFT_MODES_DTYPE is _lib.AIRCRAFT_MODES_DTYPE
    assert lib.AIRCRAFT_MODES_DTYPE.names == M.MODEL_DTYPE.names
    for name, off in M.OFFSETS.items():
        assert getattr(_lib.AdsbAircraftModes, name).offset == off == lib.AIRCRAFT_MODES_DTYPE.fields[name][1], name


def test_header_struct_flags_and_abi_version():
    """The header's struct, laid out by the C rules from its own text; the ABI version is still 1."""
    header = open(os.path.join(ROOT, "include", "adsb_hip.h")).read()
    assert "Mode S replies per aircraft" in header
    assert re.search(r"#define\s+ADSB_ABI_VERSION\s+1u?\b", header)
    assert re.search(r"static_assert\(sizeof\(adsb_aircraft_modes\) == 64", header)
    header = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    body = re.search(r"typedef\s+struct\s+adsb_aircraft_modes\s*\{(.*?)\}\s*adsb_aircraft_modes\s*;", header, re.S).group(1)
    out, off, align = {}, 0, 1
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        ctype, names = decl.split(" ", 1)
        for item in names.split(","):
            item = item.strip()
            count = 1
            m = re.match(r"(\w+)\[(\d+)\]$", item)
            if m:
                item, count = m.group(1), int(m.group(2))
            size = C_SIZE[ctype]
            align = max(align, size)
            off = (off + size - 1) // size * size
            out[item] = off
            off += size * count
    assert (out, (off + align - 1) // align * align) == (M.OFFSETS, 64)
    for name, value in (("ALT", M.ALT), ("SQUAWK", M.SQUAWK), ("GROUND", M.GROUND), ("ALERT", M.ALERT), ("SPI", M.SPI),
                        ("CALLSIGN", M.CALLSIGN), ("STATUS", M.STATUS), ("SQUITTER", M.SQUITTER)):
        assert int(re.search(r"#define\s+ADSB_TRACK_MODES_" + name + r"\s+(0x[0-9a-fA-F]+)u", header).group(1), 16) == value
        modes_bit = re.search(r"#define\s+ADSB_MODES_" + name + r"\s+(0x[0-9a-fA-F]+)u", header)
        assert (modes_bit is None) == (name in ("STATUS", "SQUITTER"))
        if modes_bit:                                                     # the shared bits keep ADSB_MODES_*'s values
            assert int(modes_bit.group(1), 16) == value
    assert int(re.search(r"#define\s+ADSB_TRACK_UNADDRESSED\s+(0x[0-9a-fA-F]+)u", header).group(1), 16) == 4
    assert not re.search(r"adsb_track_bank_\w*modes", header)             # tables only


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
    for method in ("modes_reserve", "modes", "modes_device"):
        assert callable(getattr(lib.TrackTable, method, None)), method
        assert not hasattr(lib.TrackBank, method), method
    assert callable(lib.host_track_modes_of) and callable(lib.host_track_modes_merge)
    sources = open(os.path.join(ROOT, "air_rs_amd", "csrc", "sources.list")).read().split()
    assert "host/adsb_track_modes.cpp" in sources
    assert (lib.ADSB_TRACK_MODES_ALT, lib.ADSB_TRACK_MODES_SQUAWK, lib.ADSB_TRACK_MODES_GROUND, lib.ADSB_TRACK_MODES_ALERT,
            lib.ADSB_TRACK_MODES_SPI, lib.ADSB_TRACK_MODES_CALLSIGN, lib.ADSB_TRACK_MODES_STATUS,
            lib.ADSB_TRACK_MODES_SQUITTER, lib.ADSB_TRACK_UNADDRESSED) == (1, 4, 8, 16, 32, 64, 256, 512, 4)
    for name in ("AIRCRAFT_MODES_DTYPE", "host_track_modes_of", "host_track_modes_merge", "ADSB_TRACK_UNADDRESSED"):
        assert name in lib.__all__, name


def test_bad_arguments(lib):
    from air_rs_amd import _lib
    L = _lib.load()
    fake = C.create_string_buffer(4096)                           # never dereferenced: every check below fails first
    h = C.addressof(fake)
    n, dev = C.c_size_t(), C.c_void_p()
    some = C.create_string_buffer(64)
    p = C.addressof(some)
    assert L.adsb_track_table_modes_reserve(None) == lib.ADSB_E_ARG
    assert L.adsb_track_table_update_modes(None, p, p, None, None, 1, 0) == lib.ADSB_E_ARG
    assert L.adsb_track_table_update_modes(None, None, None, None, None, 0, 0) == lib.ADSB_E_ARG
    assert L.adsb_track_table_update_modes(h, None, p, None, None, 1, 0) == lib.ADSB_E_ARG
    assert L.adsb_track_table_update_modes(h, p, None, None, None, 1, 0) == lib.ADSB_E_ARG
    assert L.adsb_track_table_update_modes(h, None, None, p, p, 1, 0) == lib.ADSB_E_ARG
    assert L.adsb_track_table_fetch_modes(None, None, 0, C.byref(n)) == lib.ADSB_E_ARG
    assert L.adsb_track_table_fetch_modes(h, None, 4, C.byref(n)) == lib.ADSB_E_ARG
    assert L.adsb_track_table_modes_device(None, C.byref(dev)) == lib.ADSB_E_ARG
