"""The CPU mirror of the track table's mlat step (adsb_host_track_mlat_of) against the independent model
(tests/track_mlat_model.py) on tests/track_mlat_cases.py, and the model's merge pinned by hand (CPU tier).

Integer fields, flags, times and everything copied from the fix are equal bit for bit.  disagreement_m: the largest gap
between mirror and model over all cases was measured (profiles/track_mlat_checks.txt) and is GAP_M; the tolerance is ten
times that gap, or one f32 step of the expected value where the gap is 0: the project's rule for mlat and clock sync."""
import math

import numpy as np

import air_rs_amd as A
from tests import track_mlat_cases as K
from tests import track_mlat_model as M

GAP_M = 0.0                      # measured: mirror and model agree to the bit on every case


def tol_of(want):
    return 10.0 * GAP_M if GAP_M > 0.0 else M.f32_step(want)


def test_dtypes_are_the_models():
    assert A.AIRCRAFT_MLAT_DTYPE.itemsize == 64 and A.FRAME_MLAT_DTYPE.itemsize == 16
    for name, off in M.OFFSETS.items():
        assert A.AIRCRAFT_MLAT_DTYPE.fields[name][1] == off, name
    assert [A.FRAME_MLAT_DTYPE.fields[n][1] for n in M.FRAME_DTYPE.names] == [0, 4, 8, 12]
    assert A.MLAT_FIX_DTYPE == M.FIX_DTYPE


def test_mirror_equals_model_on_every_case():
    cases = K.cases()
    names = [c[0] for c in cases]
    assert len(set(names)) == len(names) > 500
    seen = {"checked": 0, "disagree": 0, "far": 0, "valid unchecked": 0, "not valid": 0, "agree": 0}
    gap = 0.0
    for name, limit, frame, fx, time in cases:
        got, flags, dis = A.host_track_mlat_of(limit, frame, fx, time)
        want, want_flags, want_dis = M.record_of(limit, frame, fx, time)
        assert flags == want_flags, (name, flags, want_flags)
        gap = max(gap, abs(float(dis) - float(want_dis)))
        assert abs(float(dis) - float(want_dis)) <= tol_of(want_dis), (name, dis, want_dis)
        M.assert_records_equal(np.array([got]).view(M.MODEL_DTYPE), np.array([want]), tol_of, name)
        # the planted disagreements keep clear of their limit by far more than the tolerance
        if flags & M.CHECKED and not flags & M.FAR:
            assert abs(float(want_dis) - limit) > 0.3 * min(limit, float(want_dis)) + 1e-4, (name, want_dis, limit)
        assert bool(flags & M.CHECKED) == bool(got["flags"] & M.CHECKED) and got["n_checked"] == bool(flags & M.CHECKED)
        assert got["n_disagree"] == bool(flags & M.DISAGREE) and got["n_valid"] == bool(flags & M.VALID)
        assert got["n_attempted"] == bool(int(fx["flags"]) & M.FIX_ATTEMPTED)
        if not flags & M.VALID:
            assert got.tobytes()[8:44] == bytes(36) and math.isnan(got["time"]) and dis == 0.0
        seen["checked"] += bool(flags & M.CHECKED)
        seen["disagree"] += bool(flags & M.DISAGREE)
        seen["far"] += bool(flags & M.FAR)
        seen["agree"] += flags & (M.CHECKED | M.DISAGREE) == M.CHECKED
        seen["valid unchecked"] += flags == M.VALID
        seen["not valid"] += flags == 0
    print("largest gap between mirror and model:", gap, "m over", len(cases), "cases;", seen)
    assert seen["far"] >= 8 and seen["agree"] > 100 and seen["disagree"] > 100 and seen["valid unchecked"] > 50
    assert seen["not valid"] >= 12


def test_honest_and_displaced_frames_land_where_they_were_planted():
    for name, limit, frame, fx, time in K.cases():
        if not name.startswith("tc "):
            continue
        tc, shift = int(name.split()[1]), float(name.split()[4])
        flags, dis, _ = M.frame_check(limit, frame, fx)
        if 9 <= tc <= 18 or 20 <= tc <= 22:
            assert flags & M.CHECKED and (float(dis) < 50.0 if shift < 100 else 2000.0 < float(dis) < 8000.0), (name, dis)
            assert bool(flags & M.DISAGREE) == (shift > 100)
        else:
            assert flags == M.VALID, name


def test_mirror_argument_errors(lib):
    import ctypes as C
    from air_rs_amd import _lib
    L = _lib.load()
    b = (C.c_uint8 * 14)()
    fx, out = _lib.AdsbMlatFix(), _lib.AdsbAircraftMlat()
    call = L.adsb_host_track_mlat_of
    assert call(1000.0, C.byref(b), C.byref(fx), 0.0, C.byref(out), None, None) == lib.ADSB_OK
    assert call(1000.0, None, C.byref(fx), 0.0, C.byref(out), None, None) == lib.ADSB_E_ARG
    assert call(1000.0, C.byref(b), None, 0.0, C.byref(out), None, None) == lib.ADSB_E_ARG
    assert call(1000.0, C.byref(b), C.byref(fx), 0.0, None, None, None) == lib.ADSB_E_ARG
    for bad in (0.0, -1.0, math.nan, math.inf, -math.inf):
        assert call(bad, C.byref(b), C.byref(fx), 0.0, C.byref(out), None, None) == lib.ADSB_E_ARG, bad


def test_model_merge_by_hand():
    """Newest valid wins, an invalid fix leaves the kept one, the check's newest and maximum, a cut changes nothing,
    the counts saturate."""
    icao, place = 0x4B1234, (47.0, 8.0)
    near = M.position_frame(icao, 11, 0, *place)
    away = M.position_frame(icao, 11, 1, 47.05, 8.0)                       # 0.05 degrees of latitude: 5.56 km
    vel = M.raw_frame(icao, 19 << 51 | 1 << 48)
    items = [(100, near), (200, vel), (200, away), (300, near), (400, vel), (500, M.position_frame(0x4B0001, 11, 0, 1.0, 2.0))]
    fixes = np.array([M.fix(*place, height_m=1000.0), M.fix(*place, height_m=2000.0, flags=K.GOOD | M.FIX_ALTITUDE),
                      M.fix(*place, height_m=3000.0), M.fix(0.0, 0.0, flags=0x1 | 0x20), M.fix(0.0, 0.0, flags=0x8),
                      M.fix(1.0, 2.0, flags=0x8)])
    frames = M.frames_array(items, np.dtype([("offset", "<u8"), ("bytes", "u1", (14,))]))
    st = M.apply({}, 1000.0, frames, fixes, sample_base=50, sps=0.5)
    a = st[icao]
    assert (a["n_attempted"], a["n_valid"], a["n_checked"], a["n_disagree"], a["n_used"]) == (4, 3, 2, 1, 5)
    assert a["time"] == 125.0 and a["height_m"] == 3000.0 and a["flags"] == M.VALID | M.CHECKED   # the third, not ALTITUDE
    assert 5500.0 < a["last_disagreement_m"] == a["max_disagreement_m"] < 5620.0
    b = st[0x4B0001]
    assert b.tobytes() == M.empty().tobytes() and b.tobytes()[8:] == bytes(56)
    one = M.apply({}, 1000.0, frames[:2], fixes[:2], 50, 0.5)[icao]
    assert one["flags"] == M.VALID | M.ALTITUDE | M.CHECKED and one["last_disagreement_m"] < 10.0 and one["time"] == 125.0
    two = M.apply(M.apply({}, 1000.0, frames[:3], fixes[:3], 50, 0.5), 1000.0, frames[3:], fixes[3:], 50, 0.5)
    assert M.records(two, sorted(two)).tobytes() == M.records(st, sorted(st)).tobytes()
    full = a.copy()
    for name in ("n_attempted", "n_valid", "n_checked", "n_disagree"):
        full[name] = M.U32
    sat = M.apply({icao: full}, 1000.0, frames[:3], fixes[:3], 50, 0.5)[icao]
    assert all(sat[name] == M.U32 for name in ("n_attempted", "n_valid", "n_checked", "n_disagree"))
