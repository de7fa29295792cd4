"""Airborne velocity in the track table and bank (adsb_track_*_fetch_velocity): the 32-byte adsb_velocity layout, its
flags, argument checks before any device access, and the NumPy model against two known answers (CPU tier)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from tests.velocity_traffic import DIRECTION, MODEL_DTYPE, SPEED, VRATE, decode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("adsb_track_table_fetch_velocity", "adsb_track_bank_fetch_velocity")
OFFSETS = {"time": 0, "speed_kt": 8, "direction_deg": 12, "vertical_rate_fpm": 16, "v_ew_kt": 20, "v_ns_kt": 22,
           "subtype": 24, "flags": 25, "vrate_baro": 26, "airspeed_tas": 27, "reserved": 28}
# CRC-valid DF17 TC 19 frames (ST 1: ground speed, ST 3: airspeed and heading) and what they decode to
KNOWN_ST1 = "8D485020994409940838175B284F"
KNOWN_ST3 = "8DA05F219B06B6AF189400CBC33F"


def test_velocity_struct_layout(lib):
    from air_rs_amd import _lib
    assert C.sizeof(_lib.AdsbVelocity) == 32 and lib.VELOCITY_DTYPE.itemsize == 32
    for name, off in OFFSETS.items():
        assert getattr(_lib.AdsbVelocity, name).offset == off, name
        assert lib.VELOCITY_DTYPE.fields[name][1] == off, name
    assert lib.VELOCITY_DTYPE == MODEL_DTYPE


def test_velocity_constants_and_declarations(lib):
    from air_rs_amd import _lib
    assert (lib.ADSB_VELOCITY_SPEED, lib.ADSB_VELOCITY_DIRECTION, lib.ADSB_VELOCITY_VRATE) == (SPEED, DIRECTION, VRATE)
    header = open(os.path.join(ROOT, "include", "adsb_hip.h")).read()
    for name, value in (("SPEED", 1), ("DIRECTION", 2), ("VRATE", 4)):
        assert re.search(r"#define ADSB_VELOCITY_" + name + r"\s+0x" + str(value) + "u", header), name
    L = _lib.load()
    for name in NEW:
        assert hasattr(L, name) and name in _lib.PROTOTYPES, name
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
    for cls in (lib.TrackTable, lib.TrackBank):
        assert callable(getattr(cls, "velocity", None)), cls


def test_velocity_bad_arguments(lib):
    from air_rs_amd import _lib
    L = _lib.load()
    fake = C.create_string_buffer(64)                             # never dereferenced: every check below fails first
    n = C.c_size_t(123)
    out = (_lib.AdsbVelocity * 4)()
    for fn in (L.adsb_track_table_fetch_velocity, L.adsb_track_bank_fetch_velocity):
        assert fn(None, out, 4, C.byref(n)) == lib.ADSB_E_ARG
        assert fn(None, None, 0, C.byref(n)) == lib.ADSB_E_ARG
        assert fn(C.addressof(fake), None, 4, C.byref(n)) == lib.ADSB_E_ARG
    assert n.value == 123                                         # untouched by a rejected call


def test_model_known_answers():
    v = decode(bytes.fromhex(KNOWN_ST1), 1.5)
    assert v["time"] == 1.5 and v["subtype"] == 1 and v["flags"] == SPEED | DIRECTION | VRATE
    assert (int(v["v_ew_kt"]), int(v["v_ns_kt"])) == (-8, -159)
    assert v["speed_kt"] == np.float32(math.sqrt(8 * 8 + 159 * 159))
    assert float(v["speed_kt"]) == pytest.approx(159.2011, abs=1e-4)
    assert float(v["direction_deg"]) == pytest.approx(182.8804, abs=1e-4)
    assert int(v["vertical_rate_fpm"]) == -832 and v["vrate_baro"] == 0 and v["airspeed_tas"] == 0
    v = decode(bytes.fromhex(KNOWN_ST3), 2.0)
    assert v["subtype"] == 3 and v["flags"] == SPEED | DIRECTION | VRATE
    assert v["direction_deg"] == np.float32(243.984375) and v["speed_kt"] == np.float32(375.0)
    assert v["airspeed_tas"] == 1 and int(v["vertical_rate_fpm"]) == -2304 and v["vrate_baro"] == 1
    assert (int(v["v_ew_kt"]), int(v["v_ns_kt"])) == (0, 0)
    # not velocity messages: another type code, or TC 19 with subtype 0 / 5-7
    assert decode(bytes.fromhex("8D40621D58C386435CC412692AD6"), 0.0) is None
    me = bytearray(bytes.fromhex(KNOWN_ST1))
    for st in (0, 5, 6, 7):
        me[4] = 19 << 3 | st
        assert decode(bytes(me), 0.0) is None, st
