"""Per-aircraft signal levels (adsb_track_*_levels_*, adsb_fused_level): the two layouts, the declarations, the argument
checks that need no device, and the Python model (tests/track_levels_model.py) against hand-made inputs with known
answers, so the model is pinned by something other than the code it judges on the GPU (CPU tier)."""
import ctypes as C
import math
import os
import re

import numpy as np

from tests import track_levels_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("adsb_track_table_levels_reserve", "adsb_track_table_update_levels", "adsb_track_table_fetch_levels",
       "adsb_track_table_levels_device", "adsb_track_bank_levels_reserve", "adsb_track_bank_update_levels",
       "adsb_track_bank_update_launch_levels", "adsb_track_bank_fetch_levels", "adsb_track_bank_levels_device",
       "adsb_track_bank_fetch_fused_levels")
C_SIZE = {"double": 8, "uint64_t": 8, "uint32_t": 4, "uint16_t": 2}


def test_struct_layouts(lib):
    from air_rs_amd import _lib
    assert C.sizeof(_lib.AdsbAircraftLevel) == 64 == lib.AIRCRAFT_LEVEL_DTYPE.itemsize
    assert C.sizeof(_lib.AdsbFusedLevel) == 96 == lib.FUSED_LEVEL_DTYPE.itemsize
    for name, off in M.OFFSETS.items():
        assert getattr(_lib.AdsbAircraftLevel, name).offset == off, name
        assert lib.AIRCRAFT_LEVEL_DTYPE.fields[name][1] == off, name
    for name, off in M.FUSED_OFFSETS.items():
        assert getattr(_lib.AdsbFusedLevel, name).offset == off, name
        assert lib.FUSED_LEVEL_DTYPE.fields[name][1] == off, name
    assert lib.AIRCRAFT_LEVEL_DTYPE == M.MODEL_DTYPE and lib.FUSED_LEVEL_DTYPE == M.FUSED_DTYPE
    assert lib.LEVEL_DTYPE == M.FRAME_LEVEL


def test_header_structs_have_the_documented_offsets():
    """The header's two structs, laid out by the C rules from its own text; adsb_fused_level spells its level record
    out field by field, as adsb_fused_aircraft does its velocity: the same names with strongest_ in front, in order."""
    header = open(os.path.join(ROOT, "include", "adsb_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)

    def fields(struct):
        body = re.search(r"typedef\s+struct\s+" + struct + r"\s*\{(.*?)\}\s*" + struct + r"\s*;", header, re.S).group(1)
        out, off = {}, 0
        for decl in body.split(";"):
            decl = " ".join(decl.split())
            if not decl:
                continue
            ctype, names = decl.split(" ", 1)
            for item in names.split(","):
                size = C_SIZE[ctype]
                off = (off + size - 1) // size * size
                out[item.strip()] = off
                off += size
        return out, off

    assert fields("adsb_aircraft_level") == (M.OFFSETS, 64)
    want = {"strongest_" + name: off for name, off in M.OFFSETS.items()}
    want.update({name: off for name, off in M.FUSED_OFFSETS.items() if name != "strongest"})
    got, size = fields("adsb_fused_level")
    assert (got, size) == (want, 96) and list(got)[:10] == ["strongest_" + name for name in M.OFFSETS]


def test_declarations(lib):
    from air_rs_amd import _lib
    header = open(os.path.join(ROOT, "include", "adsb_hip.h")).read()
    L = _lib.load()
    for name in NEW:
        assert hasattr(L, name) and name in _lib.PROTOTYPES, name
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
    for cls in (lib.TrackTable, lib.TrackBank):
        for method in ("levels_reserve", "levels", "levels_device"):
            assert callable(getattr(cls, method, None)), (cls, method)
    assert callable(lib.TrackBank.fused_levels)


def test_null_handles(lib):
    from air_rs_amd import _lib
    L = _lib.load()
    n = C.c_size_t()
    dev = C.c_void_p()
    assert L.adsb_track_table_levels_reserve(None) == lib.ADSB_E_ARG
    assert L.adsb_track_table_update_levels(None, None, None, 0, 0) == lib.ADSB_E_ARG
    assert L.adsb_track_table_fetch_levels(None, None, 0, C.byref(n)) == lib.ADSB_E_ARG
    assert L.adsb_track_table_levels_device(None, C.byref(dev)) == lib.ADSB_E_ARG
    assert L.adsb_track_bank_levels_reserve(None) == lib.ADSB_E_ARG
    assert L.adsb_track_bank_update_levels(None, None, None, 0, None, None) == lib.ADSB_E_ARG
    assert L.adsb_track_bank_update_launch_levels(None, None) == lib.ADSB_E_ARG
    assert L.adsb_track_bank_fetch_levels(None, None, 0, C.byref(n)) == lib.ADSB_E_ARG
    assert L.adsb_track_bank_levels_device(None, C.byref(dev)) == lib.ADSB_E_ARG
    assert L.adsb_track_bank_fetch_fused_levels(None, None, 0, C.byref(n)) == lib.ADSB_E_ARG


# ---- the model, pinned by hand ------------------------------------------------------------------------------------------
def _frames(items):
    """[(offset, icao)] -> an array with the two fields of adsb_frame the model reads."""
    out = np.zeros(len(items), dtype=[("offset", "<u8"), ("bytes", "u1", (14,))])
    for k, (off, icao) in enumerate(items):
        out[k]["offset"] = off
        out[k]["bytes"][0] = 0x8D
        out[k]["bytes"][1:4] = [(icao >> 16) & 0xFF, (icao >> 8) & 0xFF, icao & 0xFF]
    return out


def _levels(rows):
    """[(signal_sum, noise_sum, peak, weak_bits, flags)]"""
    out = np.zeros(len(rows), dtype=M.FRAME_LEVEL)
    for k, (s, q, p, w, f) in enumerate(rows):
        out[k]["signal_sum"], out[k]["noise_sum"], out[k]["peak"], out[k]["weak_bits"], out[k]["flags"] = s, q, p, w, f
    return out


def test_model_sums_maxima_and_newest_by_list_order():
    frames = _frames([(100, 0xABCDEF), (200, 0x000001), (200, 0xABCDEF), (200, 0xABCDEF), (300, 0xABCDEF)])
    levels = _levels([(10, 1, 7, 2, 1), (99, 9, 9, 9, 1), (30, 3, 5, 1, 1), (20, 2, 6, 0, 1), (1000, 1000, 1000, 100, 0)])
    st = M.apply({}, frames, levels, sample_base=50, sps=0.5)
    a = st[0xABCDEF]
    assert (a["signal_total"], a["noise_total"], a["n_levels"], a["peak"], a["weak_bits_total"]) == (60, 6, 3, 7, 3)
    assert a["max_signal_sum"] == 30
    # equal offsets: the later one in list order is the newest; the invalid frame at 300 is not counted
    assert (a["last_signal_sum"], a["last_noise_sum"], a["last_time"]) == (20, 2, 125.0)
    rec = M.records(st, [0x000001, 0x777777, 0xABCDEF])
    assert rec.dtype.itemsize == 64 and rec[0]["signal_total"] == 99 and rec[2]["last_time"] == 125.0
    assert rec[1].tobytes() == M.records({}, [5])[0].tobytes() and math.isnan(rec[1]["last_time"])
    assert rec[1].tobytes()[:40] == bytes(40) and rec[1].tobytes()[48:] == bytes(16)
    # a cut changes nothing
    two = M.apply(M.apply({}, frames[:3], levels[:3], 50, 0.5), frames[3:], levels[3:], 50, 0.5)
    assert M.records(two, sorted(two)).tobytes() == M.records(st, sorted(st)).tobytes()
    # an untracked frame is not counted
    un = M.apply({}, frames, levels, 50, 0.5, untracked=[False, True, False, False, False])
    assert 0x000001 not in un and un[0xABCDEF] == a


def test_model_saturates():
    frames = _frames([(k, 7) for k in range(3)])
    levels = _levels([(1 << 63, M.U64, 5, 65535, 1), (1 << 63, 1, 4, 65535, 1), (3, 0, 1, 0, 1)])
    a = M.apply({}, frames, levels)[7]
    assert a["signal_total"] == M.U64 and a["noise_total"] == M.U64
    assert a["max_signal_sum"] == 1 << 63 and a["last_signal_sum"] == 3 and a["n_levels"] == 3
    a["n_levels"], a["weak_bits_total"] = M.U32, M.U32 - 1
    st = M.apply({7: a}, frames[:1], levels[:1])
    assert st[7]["n_levels"] == M.U32 and st[7]["weak_bits_total"] == M.U32
    assert M.records(st, [7])[0]["signal_total"] == M.U64


def _lv(total, n, noise=0):
    r = M.records({}, [0])[0].copy()
    r["signal_total"], r["n_levels"], r["noise_total"], r["last_time"] = total, n, noise, 1.0
    return r


def test_model_strongest_and_ties():
    icaos = [np.array([5, 9]), np.array([5, 9]), np.array([9])]
    heard = [np.array([1.0, 1.0]), np.array([2.0, 0.5]), np.array([3.0])]
    levels = [np.array([_lv(4, 2), _lv(2, 1, 10)]), np.array([_lv(2, 1), _lv(4, 2, 20)]), np.array([_lv(0, 0, 0)])]
    out = M.fuse(icaos, heard, levels)
    assert list(out["strongest_receiver"]) == [0, 0] and list(out["level_receivers"]) == [2, 2]
    assert list(out["signal_total"]) == [6, 6] and list(out["n_levels"]) == [3, 3] and list(out["noise_total"]) == [0, 30]
    assert out[0]["strongest"].tobytes() == levels[0][0].tobytes()
    # since drops receiver 1's record of ICAO 9: receiver 0 alone
    out = M.fuse(icaos, heard, levels, since=1.0)
    assert list(out["strongest_receiver"]) == [0, 0] and list(out["level_receivers"]) == [2, 1]
    # nobody has a level: NONE and an empty record
    out = M.fuse([np.array([9])], [np.array([3.0])], [np.array([_lv(0, 0)])])
    assert out[0]["strongest_receiver"] == M.NONE and math.isnan(out[0]["strongest"]["last_time"])
    assert out[0]["level_receivers"] == 0
    # means a double cannot tell apart: (2^62 + 2^31) / 2^31 = 2^31 + 1, and 2^62 - 1 = (2^31 - 1)(2^31 + 1), so
    # (2^62 - 1) / (2^31 - 1) is an exact tie with it and 2^62 / (2^31 - 1) is greater by 1 / (2^31 - 1)
    a, b = _lv((1 << 62) - 1, (1 << 31) - 1), _lv((1 << 62) + (1 << 31), 1 << 31)
    assert not M.stronger(a, b) and not M.stronger(b, a)
    assert M.stronger(_lv(1 << 62, (1 << 31) - 1), b) and not M.stronger(b, _lv(1 << 62, (1 << 31) - 1))
    assert float(1 << 62) / float((1 << 31) - 1) == float((1 << 62) + (1 << 31)) / float(1 << 31)   # what f64 sees
    out = M.fuse([np.array([1])] * 2, [np.array([0.0])] * 2, [np.array([b]), np.array([_lv(1 << 62, (1 << 31) - 1)])])
    assert out[0]["strongest_receiver"] == 1 and out[0]["n_levels"] == (1 << 32) - 1
    out = M.fuse([np.array([1])] * 2, [np.array([0.0])] * 2, [np.array([b]), np.array([a])])
    assert out[0]["strongest_receiver"] == 0
    # the fused totals saturate
    out = M.fuse([np.array([1])] * 2, [np.array([0.0])] * 2, [np.array([_lv(M.U64, 3)]), np.array([_lv(5, 1)])])
    assert out[0]["signal_total"] == M.U64 and out[0]["strongest_receiver"] == 0
