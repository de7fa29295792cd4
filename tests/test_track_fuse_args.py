"""The fused view of a track bank (adsb_track_bank_fuse_*, TrackBank.fuse): the 128-byte adsb_fused_aircraft layout,
argument checks that need no device, and the NumPy model (tests/fuse_model.py) against hand-made records with known
answers, so the model is pinned by something other than the code it judges on the GPU (CPU tier)."""
import ctypes as C
import os
import re

import numpy as np

from tests import fuse_model
from tests.fuse_model import NONE, OFFSETS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("adsb_track_bank_fuse_reserve", "adsb_track_bank_fuse", "adsb_track_bank_fetch_fused",
       "adsb_track_bank_fused_device")
# the header's field names, in order, with their offsets: the eleven from velocity_time on are an adsb_velocity
HEADER_FIELDS = [("latitude", 0), ("longitude", 8), ("position_time", 16), ("last_contact", 24), ("last_heard", 32),
                 ("n_frames", 40), ("icao", 48), ("altitude", 52), ("n_receivers", 56), ("heard_receiver", 58),
                 ("contact_receiver", 60), ("position_receiver", 62), ("callsign_receiver", 64),
                 ("velocity_receiver", 66), ("has_position", 68), ("callsign", 72), ("velocity_time", 80),
                 ("speed_kt", 88), ("direction_deg", 92), ("vertical_rate_fpm", 96), ("v_ew_kt", 100),
                 ("v_ns_kt", 102), ("velocity_subtype", 104), ("velocity_flags", 105), ("vrate_baro", 106),
                 ("airspeed_tas", 107), ("velocity_reserved", 108), ("reserved", 112)]
C_SIZE = {"double": 8, "float": 4, "uint64_t": 8, "uint32_t": 4, "int32_t": 4, "uint16_t": 2, "int16_t": 2,
          "uint8_t": 1, "char": 1}


def test_fused_struct_layout(lib):
    from air_rs_amd import _lib
    assert C.sizeof(_lib.AdsbFusedAircraft) == 128 and lib.FUSED_DTYPE.itemsize == 128
    for name, off in OFFSETS.items():
        assert getattr(_lib.AdsbFusedAircraft, name).offset == off, name
        assert lib.FUSED_DTYPE.fields[name][1] == off, name
    assert lib.FUSED_DTYPE == fuse_model.MODEL_DTYPE
    assert lib.FUSED_DTYPE.fields["velocity"][0] == lib.VELOCITY_DTYPE


def test_fused_header_struct_is_128_bytes_with_the_documented_offsets():
    """The header's struct, laid out by the C rules from its own text: every field at the documented offset, naturally
    aligned, 128 bytes; its velocity fields are adsb_velocity's, in order, at offset 80."""
    header = open(os.path.join(ROOT, "include", "adsb_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)

    def fields(struct):
        body = re.search(r"typedef\s+struct\s+" + struct + r"\s*\{(.*?)\}\s*" + struct + r"\s*;", header, re.S).group(1)
        out, off = [], 0
        for decl in body.split(";"):
            decl = " ".join(decl.split())
            if not decl:
                continue
            ctype, names = decl.split(" ", 1)
            for item in names.split(","):
                m = re.match(r"\s*(\w+)\s*(?:\[(\d+)\])?\s*$", item)
                size = C_SIZE[ctype]
                off = (off + size - 1) // size * size
                out.append((m.group(1), off, ctype))
                off += size * int(m.group(2) or 1)
        return out, off

    got, size = fields("adsb_fused_aircraft")
    assert size == 128
    assert [(n, o) for n, o, _ in got] == HEADER_FIELDS
    vel, vel_size = fields("adsb_velocity")
    assert vel_size == 32
    mine = [(o - 80, t) for n, o, t in got if 80 <= o < 112]
    assert mine == [(o, t) for _, o, t in vel]
    assert re.search(r"#define ADSB_FUSED_NONE\s+0xFFFFu", header)
    assert re.search(r"#define ADSB_TRACK_FUSED_TRUNCATED\s+0x1u", header)


def test_fused_constants_and_declarations(lib):
    from air_rs_amd import _lib
    assert lib.ADSB_FUSED_NONE == NONE == 0xFFFF and lib.ADSB_TRACK_FUSED_TRUNCATED == 1
    header = open(os.path.join(ROOT, "include", "adsb_hip.h")).read()
    L = _lib.load()
    for name in NEW:
        assert hasattr(L, name) and name in _lib.PROTOTYPES, name
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
    for method in ("fuse", "fuse_reserve", "fused_device"):
        assert callable(getattr(lib.TrackBank, method, None)), method


def test_fused_bad_arguments(lib):
    from air_rs_amd import _lib
    L = _lib.load()
    n, total, flags = C.c_size_t(123), C.c_size_t(456), C.c_uint32(789)
    out = (_lib.AdsbFusedAircraft * 4)()
    rec, counts = C.c_void_p(), C.c_void_p()
    assert L.adsb_track_bank_fuse_reserve(None, 0) == lib.ADSB_E_ARG
    assert L.adsb_track_bank_fuse_reserve(None, 1000) == lib.ADSB_E_ARG
    assert L.adsb_track_bank_fuse(None, 0.0) == lib.ADSB_E_ARG
    assert L.adsb_track_bank_fuse(None, float("-inf")) == lib.ADSB_E_ARG
    assert L.adsb_track_bank_fetch_fused(None, out, 4, C.byref(n), C.byref(total), C.byref(flags)) == lib.ADSB_E_ARG
    assert L.adsb_track_bank_fetch_fused(None, None, 0, C.byref(n), C.byref(total), C.byref(flags)) == lib.ADSB_E_ARG
    assert L.adsb_track_bank_fused_device(None, C.byref(rec), C.byref(counts)) == lib.ADSB_E_ARG
    assert (n.value, total.value, flags.value) == (123, 456, 789)   # untouched by a rejected call
    assert rec.value is None and counts.value is None


# ---- the model against hand-made records with known answers ---------------------------------------------------------
def _bank(lib, n_receivers):
    return ([[] for _ in range(n_receivers)], [[] for _ in range(n_receivers)], [[] for _ in range(n_receivers)])


def _put(lib, bank, r, icao, heard, contact=np.nan, pos=None, alt=0, callsign=b"", n_frames=1, vel=None):
    """One record on receiver r; vel = (time, subtype, speed)."""
    rec = np.zeros((), dtype=lib.AIRCRAFT_DTYPE)
    rec["icao"], rec["last_contact"], rec["altitude"], rec["n_frames"], rec["callsign"] = icao, contact, alt, n_frames, callsign
    if pos is not None:
        rec["has_position"], rec["latitude"], rec["longitude"] = 1, pos[0], pos[1]
    v = np.zeros((), dtype=lib.VELOCITY_DTYPE)
    v["time"] = np.nan
    if vel is not None:
        v["time"], v["subtype"], v["speed_kt"], v["flags"] = vel[0], vel[1], vel[2], 1
    bank[0][r].append(rec)
    bank[1][r].append(heard)
    bank[2][r].append(v)


def _run(lib, bank, since=-np.inf):
    recs = [np.array(x, dtype=lib.AIRCRAFT_DTYPE) for x in bank[0]]
    for x in recs:
        assert list(x["icao"]) == sorted(x["icao"])                # as aircraft() returns them
    return fuse_model.fuse(recs, [np.array(x, dtype=np.float64) for x in bank[1]],
                           [np.array(x, dtype=lib.VELOCITY_DTYPE) for x in bank[2]], since)


def test_model_every_quantity_from_a_different_receiver(lib):
    """One ICAO on three receivers, times crafted so that no receiver is the answer to everything: receiver 2 heard it
    last, receiver 1 has the newest position message (no fix) and the newest callsign, receiver 0 the only fix and the
    newest velocity.  Three receivers cannot give five different answers; every neighbouring pair differs."""
    b = _bank(lib, 3)
    _put(lib, b, 0, 0xABCDEF, heard=10.0, contact=8.0, pos=(51.5, -0.1), alt=30000, callsign=b"OLD", n_frames=7,
         vel=(9.5, 1, 400.0))
    _put(lib, b, 1, 0xABCDEF, heard=11.0, contact=11.0, alt=31000, callsign=b"NEW1", n_frames=5, vel=(9.0, 3, 390.0))
    _put(lib, b, 2, 0xABCDEF, heard=12.0, n_frames=2)          # NaN contact, no callsign, no velocity
    out = _run(lib, b)
    assert len(out) == 1
    o = out[0]
    assert o["icao"] == 0xABCDEF and o["n_receivers"] == 3 and o["n_frames"] == 14
    assert (o["heard_receiver"], o["last_heard"]) == (2, 12.0)
    assert (o["contact_receiver"], o["last_contact"], o["altitude"]) == (1, 11.0, 31000)
    assert (o["position_receiver"], o["has_position"], o["latitude"], o["longitude"], o["position_time"]) == \
        (0, 1, 51.5, -0.1, 8.0)
    assert (o["callsign_receiver"], o["callsign"]) == (1, b"NEW1")
    assert (o["velocity_receiver"], o["velocity"]["time"], o["velocity"]["subtype"], o["velocity"]["speed_kt"]) == \
        (0, 9.5, 1, 400.0)
    assert list(o["reserved"]) == [0, 0]


def test_model_exact_ties_go_to_receiver_0(lib):
    b = _bank(lib, 3)
    for r in range(3):
        _put(lib, b, r, 0x400001, heard=5.0, contact=4.0, pos=(10.0 + r, 20.0 + r), alt=1000 * (r + 1),
             callsign=b"TIE%d" % r, n_frames=3, vel=(4.5, 1, 100.0 + r))
    o = _run(lib, b)[0]
    for k in ("heard_receiver", "contact_receiver", "position_receiver", "callsign_receiver", "velocity_receiver"):
        assert o[k] == 0, k
    assert (o["altitude"], o["latitude"], o["longitude"], o["callsign"], o["velocity"]["speed_kt"]) == \
        (1000, 10.0, 20.0, b"TIE0", 100.0)
    assert o["n_receivers"] == 3 and o["n_frames"] == 9
    # a tie between receivers 1 and 2 only, above receiver 0: receiver 1
    b = _bank(lib, 3)
    _put(lib, b, 0, 0x400001, heard=1.0, contact=1.0, callsign=b"A", vel=(1.0, 1, 1.0))
    _put(lib, b, 1, 0x400001, heard=2.0, contact=2.0, alt=5, callsign=b"B", vel=(2.0, 1, 2.0))
    _put(lib, b, 2, 0x400001, heard=2.0, contact=2.0, alt=6, callsign=b"C", vel=(2.0, 1, 3.0))
    o = _run(lib, b)[0]
    assert (o["heard_receiver"], o["contact_receiver"], o["callsign_receiver"], o["velocity_receiver"]) == (1, 1, 1, 1)
    assert o["position_receiver"] == NONE and (o["altitude"], o["callsign"]) == (5, b"B")


def test_model_nan_contact_and_nothing_to_report(lib):
    """A record with NaN last_contact never gives contact or altitude; alone, every optional quantity is NONE."""
    b = _bank(lib, 3)
    _put(lib, b, 1, 0x123456, heard=3.0, n_frames=4)
    o = _run(lib, b)[0]
    assert (o["heard_receiver"], o["last_heard"], o["n_receivers"], o["n_frames"]) == (1, 3.0, 1, 4)
    for k in ("contact_receiver", "position_receiver", "callsign_receiver", "velocity_receiver"):
        assert o[k] == NONE, k
    assert np.isnan(o["last_contact"]) and np.isnan(o["position_time"]) and np.isnan(o["velocity"]["time"])
    assert (o["altitude"], o["has_position"], o["latitude"], o["longitude"], o["callsign"]) == (0, 0, 0.0, 0.0, b"")
    assert o["velocity"]["subtype"] == 0 and o["velocity"]["flags"] == 0
    want = np.zeros((), dtype=fuse_model.MODEL_DTYPE)                 # and bit for bit
    want["icao"], want["last_heard"], want["n_receivers"], want["n_frames"], want["heard_receiver"] = 0x123456, 3.0, 1, 4, 1
    for k in ("contact_receiver", "position_receiver", "callsign_receiver", "velocity_receiver"):
        want[k] = NONE
    want["last_contact"] = want["position_time"] = want["velocity"]["time"] = np.nan
    assert o.tobytes() == want.tobytes()
    # next to a record with a contact, the NaN one still counts and can be heard last
    _put(lib, b, 0, 0x123456, heard=2.0, contact=2.0, alt=700)
    o = _run(lib, b)[0]
    assert (o["heard_receiver"], o["contact_receiver"], o["last_contact"], o["altitude"], o["n_receivers"]) == \
        (1, 0, 2.0, 700, 2)


def test_model_position_from_an_older_contact_than_one_without(lib):
    b = _bank(lib, 2)
    _put(lib, b, 0, 0x777777, heard=20.0, contact=20.0, alt=12000)                        # newer, no fix
    _put(lib, b, 1, 0x777777, heard=15.0, contact=15.0, pos=(-33.9, 151.2), alt=11000)    # older, has the fix
    o = _run(lib, b)[0]
    assert (o["contact_receiver"], o["last_contact"], o["altitude"]) == (0, 20.0, 12000)
    assert (o["position_receiver"], o["position_time"], o["latitude"], o["longitude"]) == (1, 15.0, -33.9, 151.2)


def test_model_since_removes_a_receivers_record(lib):
    b = _bank(lib, 3)
    _put(lib, b, 0, 0x500000, heard=5.0, contact=5.0, alt=100, callsign=b"ZERO", n_frames=10)
    _put(lib, b, 1, 0x500000, heard=9.0, contact=4.0, alt=200, n_frames=20)
    _put(lib, b, 2, 0x500000, heard=7.0, n_frames=30)
    _put(lib, b, 0, 0x500001, heard=5.0)                   # only on receiver 0: gone with since > 5
    full = _run(lib, b)
    assert [int(x) for x in full["icao"]] == [0x500000, 0x500001]
    assert (full[0]["n_receivers"], full[0]["n_frames"], full[0]["callsign"]) == (3, 60, b"ZERO")
    assert (full[1]["n_receivers"], full[1]["heard_receiver"]) == (1, 0)
    cut = _run(lib, b, since=5.0)                          # last_heard >= since: 5.0 stays
    assert cut.tobytes() == full.tobytes()
    cut = _run(lib, b, since=6.0)
    assert len(cut) == 1
    o = cut[0]
    assert (o["n_receivers"], o["n_frames"], o["callsign_receiver"], o["callsign"]) == (2, 50, NONE, b"")
    assert (o["contact_receiver"], o["altitude"], o["heard_receiver"]) == (1, 200, 1)
    assert len(_run(lib, b, since=np.inf)) == 0


def test_model_orders_by_icao_and_keeps_single_receiver_aircraft(lib):
    b = _bank(lib, 3)
    _put(lib, b, 2, 0x000001, heard=1.0, callsign=b"LOW")
    _put(lib, b, 0, 0xFFFFFF, heard=2.0, contact=2.0, pos=(1.0, 2.0))
    _put(lib, b, 1, 0x800000, heard=3.0, vel=(3.0, 2, 1200.0))
    out = _run(lib, b)
    assert [int(x) for x in out["icao"]] == [0x000001, 0x800000, 0xFFFFFF]
    assert [int(x) for x in out["heard_receiver"]] == [2, 1, 0]
    assert [int(x) for x in out["n_receivers"]] == [1, 1, 1]
    assert (out[0]["callsign_receiver"], out[1]["velocity_receiver"], out[2]["position_receiver"]) == (2, 1, 0)
