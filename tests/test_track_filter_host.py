"""The CPU mirror of the filter behind a table's multilaterated fixes (adsb_host_track_filter_operand / _step, the text
the device compiles too) against the independent model in tests/track_filter_model.py, on the lists of
tests/track_filter_cases.py.  No device.

Flags, counts and times are compared exactly.  f32 fields (heights and nis as rounded once) must be equal or
neighbours.  f64 fields are compared by the largest |a - b| / max(|a|, |b|, 1) over every case.

MEASURED here (x86-64, glibc; `pytest -s` prints it): the largest such difference between mirror and model is 2.62e-16
over the operands (rn, re and the variances) and 8.88e-16 over the records and per-frame outputs of 8 497 frames.  The
bound is one order of magnitude above the larger, BOUND = 9e-15, far below the 1e-12 the definition allows (a micrometre on
the ground): both sides are f64 with the same mathematics and differ only in the order of a few roundings."""
import ctypes as C
import math

import numpy as np
import pytest

import air_rs_amd as A
from air_rs_amd import _lib as L
from air_rs_amd import demod as D
from tests import track_filter_cases as K
from tests import track_filter_model as M

BOUND = 9e-15
assert BOUND <= 1e-12


def mirror_step(c, a, o):
    return D.host_track_filter_step(a, o, **c)


def mirror_operand(c, fx, time, counted=True):
    return D.host_track_filter_operand(fx, time, counted, **c)


def run(case, step_fn=M.step, operand_fn=M.operand, operands=None, state=None):
    """One case through the model or the mirror -> (state, frames, operands in list order)."""
    c = M.config(**case["cfg"])
    state = {} if state is None else state
    fr, ops = M.apply(c, state, case["icaos"], case["fixes"], K.times(case), operands=operands, step_fn=step_fn,
                      operand_fn=operand_fn)
    return state, fr, ops


@pytest.fixture(scope="module")
def cases():
    rng = np.random.default_rng(3)
    icaos = sorted(int(x) for x in rng.choice(np.arange(0x400000, 0x800000), size=40, replace=False))
    out = {"traffic": K.traffic(7, 5000, icaos), "rules": K.rules(), "straddle": K.straddle(), "none": K.no_usable(),
           "one aircraft": K.one_aircraft(9, 600), "two aircraft": K.traffic(11, 2000, icaos[:2]),
           "flight": K.flight(FLIGHT_SEED)[0]}
    return {name: (case, run(case)) for name, case in out.items()}


FLIGHT_SEED = 1


def test_struct_sizes_and_offsets():
    for dtype, struct, size in ((M.RECORD_DTYPE, L.AdsbAircraftFilter, 192), (M.FRAME_DTYPE, L.AdsbFrameFilter, 32),
                                (M.OPERAND_DTYPE, L.AdsbFilterOperand, 64), (M.FIX_DTYPE, L.AdsbMlatFix, 64)):
        assert dtype.itemsize == C.sizeof(struct) == size
        assert {n: dtype.fields[n][1] for n in dtype.names} == {n: getattr(struct, n).offset for n, _ in struct._fields_}
    for lib, mine in ((A.AIRCRAFT_FILTER_DTYPE, M.RECORD_DTYPE), (A.FRAME_FILTER_DTYPE, M.FRAME_DTYPE),
                      (A.FILTER_OPERAND_DTYPE, M.OPERAND_DTYPE)):
        assert lib == mine
    cfg = L.AdsbTrackFilterCfg
    assert C.sizeof(cfg) == 96 and C.sizeof(cfg) % 8 == 0 and C.sizeof(L.AdsbAircraftFilter) % 64 == 0
    names = list(M.DEFAULTS) + ["reserved"]
    assert [n for n, _ in cfg._fields_] == names
    assert [getattr(cfg, n).offset for n in names] == [8 * k for k in range(10)] + [80, 84, 88]
    assert (L.ADSB_TRACK_FILTER_RUNNING, L.ADSB_TRACK_FILTER_VELOCITY, L.ADSB_TRACK_FILTER_HEIGHT) == (M.RUNNING, M.VELOCITY, M.HEIGHT)
    assert (L.ADSB_TRACK_FILTER_USABLE, L.ADSB_TRACK_FILTER_APPLIED, L.ADSB_TRACK_FILTER_INIT, L.ADSB_TRACK_FILTER_RESET,
            L.ADSB_TRACK_FILTER_OUTLIER, L.ADSB_TRACK_FILTER_SKIPPED) == (M.USABLE, M.APPLIED, M.INIT, M.RESET, M.OUTLIER, M.SKIPPED)
    assert D.filter_empty(2).tobytes() == M.empty().tobytes() * 2


def test_defaults_are_the_headers():
    """A cfg of zeros and a NULL cfg are the table of defaults: the mirror with none given equals the model with all."""
    fx = M.fix(47.0, 8.0, 9000.0, hdop=1.5, vdop=3.0, residual_rms_m=40.0)
    o = D.host_track_filter_operand(fx, 12.5)
    assert M.compare_operands(np.array([o]).view(M.OPERAND_DTYPE), np.array([M.operand(M.config(), fx, 12.5)])) <= BOUND
    lib, out = L.load(), np.zeros(1, dtype=A.FILTER_OPERAND_DTYPE)
    f = np.array([fx]).astype(A.MLAT_FIX_DTYPE)
    assert lib.adsb_host_track_filter_operand(None, f.ctypes.data_as(C.POINTER(L.AdsbMlatFix)), 12.5, 1,
                                              out.ctypes.data_as(C.POINTER(L.AdsbFilterOperand))) == A.ADSB_OK
    assert out[0].tobytes() == o.tobytes()
    # every field is used: changing it changes an operand or a step
    base = M.config()
    for name in M.DEFAULTS:
        assert M.config(**{name: 0})[name] == base[name] and M.config(**{name: 7})[name] == 7


def test_decisions_sit_far_from_their_thresholds(cases):
    """A check of the CASES, in the model alone (no library call: it passes with or without the feature, and guards
    what the comparisons of the other tests rest on).  Planted fixes lie at least 10 x the gate out (nis >= 100 gate^2), applied ones have nis below
    gate^2 / 4, so flags are comparable bit for bit whatever the last bits of a nis are.  (The flight's noise is
    Gaussian, so there only: no nis within 1 % of gate^2.)"""
    for name, (case, (state, fr, ops)) in cases.items():
        gate2 = M.config(**case["cfg"])["gate"] ** 2
        outlier, applied = (fr["flags"] & M.OUTLIER) != 0, (fr["flags"] & M.APPLIED) != 0
        assert np.array_equal(outlier, case["planted"] & ((ops["flags"] & M.USABLE) != 0)), name
        assert not (outlier & case["honest"]).any(), name
        if name == "flight":
            assert (np.abs(fr["nis"][outlier | applied] / gate2 - 1.0) > 0.01).all()
            continue
        assert (fr["nis"][outlier] >= 100.0 * gate2).all(), (name, fr["nis"][outlier].min())
        assert (fr["nis"][applied] < gate2 / 4.0).all(), (name, fr["nis"][applied].max())
    assert sum(int(c["planted"].sum()) for c, _ in cases.values()) > 150


def test_rules_get_the_flags_written_out_by_hand(cases):
    """A check of the MODEL against flags and counts written out by hand in tests/track_filter_cases.rules (no library
    call either); test_mirror_against_model and the GPU tests then hold the library to the model on the same list."""
    case, (state, fr, ops) = cases["rules"]
    bad = np.nonzero(fr["flags"] != case["flags"])[0]
    assert len(bad) == 0, [(hex(int(case["icaos"][k])), hex(int(fr["flags"][k])), hex(int(case["flags"][k]))) for k in bad[:5]]
    rec = lambda icao: state[icao]
    a = rec(0x4D0001)
    assert (a["n_applied"], a["n_skipped"], a["run"]) == (3, 1, 4) and a["flags"] & M.VELOCITY
    assert a["time"] == float(K.BASE + 13 * K.TICKS) * K.SPS
    b = rec(0x4D0002)
    assert (b["n_applied"], b["n_reset"], b["run"]) == (2, 1, 2) and not b["flags"] & M.VELOCITY
    c = rec(0x4D0003)
    assert (c["n_applied"], c["n_outlier"], c["n_reset"], c["run"], c["outliers_run"]) == (5, 3, 1, 3, 0)
    assert abs(c["latitude"] - (47.0 + K.FAR[0])) < 1e-3 and c["last_nis"] < 4.0
    d = rec(0x4D0004)
    assert d["n_applied"] == 11 and d["longitude"] < -179.9 and 240.0 < d["v_east"] < 260.0 and abs(d["v_north"]) < 5.0
    assert rec(0x4D0005)["n_applied"] == 1 and rec(0x4D0006).tobytes() == rec(0x4D0007).tobytes() == M.empty().tobytes()
    assert rec(0x4D0008)["n_applied"] == 2
    sel = case["icaos"] == 0x4D0009
    assert [int(x) & M.HEIGHT for x in ops["flags"][sel]] == [M.HEIGHT, M.HEIGHT, 0, 0, M.HEIGHT]
    e = rec(0x4D000A)
    assert e["flags"] == M.RUNNING | M.HEIGHT and e["p_up"][0] < 50.0 ** 2 * 30.0 ** 2
    first = np.nonzero(case["icaos"] == 0x4D000A)[0][0]
    assert ops["var_v"][first] == (50.0 * max(30.0, float(case["fixes"]["residual_rms_m"][first]))) ** 2
    assert rec(0x4D000B)["n_applied"] == 3 and rec(0x4D000C)["run"] == rec(0x4D000D)["run"] == 1


def test_mirror_against_model(cases, capsys):
    worst_op, worst = 0.0, 0.0
    frames = 0
    for name, (case, (state, fr, ops)) in cases.items():
        mstate, mfr, mops = run(case, mirror_step, mirror_operand)
        worst_op = max(worst_op, M.compare_operands(mops, ops, name))
        worst = max(worst, M.compare_frames(mfr, fr, name))
        icaos = sorted(set(int(i) for i in case["icaos"]))
        assert sorted(mstate) == sorted(state)
        worst = max(worst, M.compare_records(M.records(mstate, icaos), M.records(state, icaos), name))
        # the mirror's step fed the MODEL's operands: the walk on its own
        sstate, sfr, _ = run(case, mirror_step, operands=ops)
        worst = max(worst, M.compare_frames(sfr, fr, name), M.compare_records(M.records(sstate, icaos), M.records(state, icaos)))
        frames += len(case["icaos"])
    with capsys.disabled():
        print(f"\nmirror against model over {frames} frames: operands {worst_op:.3g}, records and frames {worst:.3g}, "
              f"bound {BOUND:.3g}")
    assert worst_op <= BOUND and worst <= BOUND


def test_cuts_and_unusable_frames_leave_no_trace(cases):
    """The mirror, a list cut anywhere: the same records; a frame that is not usable or not counted changes nothing."""
    case, (state, fr, ops) = cases["two aircraft"]
    whole, wfr, _ = run(case, mirror_step, mirror_operand)
    cutstate = {}
    for lo, hi in ((0, 1), (1, 700), (700, 700), (700, 2000)):
        _, cfr, _ = run(K.cut(case, lo, hi), mirror_step, mirror_operand, state=cutstate)
        assert cfr.tobytes() == wfr[lo:hi].tobytes()
    assert all(cutstate[i].tobytes() == whole[i].tobytes() for i in whole)
    a = whole[int(case["icaos"][0])]
    o = mirror_operand(M.config(), case["fixes"][0], 1.0, counted=False)
    assert o.tobytes() == bytes(64)
    b, f = mirror_step(M.config(), a, o)
    assert b.tobytes() == a.tobytes() and f.tobytes() == bytes(32)


def test_usefulness_on_a_synthetic_flight(cases, capsys):
    """230 m/s, two straight legs and a 3 degrees/s turn, fixes every 0.5..2 s, Gaussian noise of hdop x 50 m, 5 % of the
    fixes displaced by 20 km (FLIGHT_SEED is chosen so that the MODEL alone meets the conditions below): every displaced
    fix is an OUTLIER and no honest one is, and on the straight legs the filtered position is closer to the truth, RMS,
    than the raw fixes.  Only that is asserted.  Measured (accel_h = 12 as the case sets it, every other default; 261
    fixes, 18 displaced): raw 101.5 m, filtered 64.9 m, ratio 0.64; ground speed 248.3 m/s at the min_run-th fix, and
    within 14.3 m/s RMS of 230 over the last 60 s.  With the default accel_h = 3 the turn gates out 3 honest fixes and
    the filter restarts once behind it (printed, not asserted: it is what max_outliers is for)."""
    case, truth, straight = K.flight(FLIGHT_SEED)
    _, (state, fr, ops) = cases["flight"]
    assert 10 <= case["planted"].sum() and len(case["icaos"]) > 200
    for flags in (fr["flags"], run(case, mirror_step, mirror_operand)[1]["flags"]):
        outlier = (flags & M.OUTLIER) != 0
        assert np.array_equal(outlier, case["planted"]) and not (flags & (M.RESET | M.SKIPPED)).any()
    metres = lambda lat, lon: np.hypot((lat - truth[:, 0]) * 111_000.0,
                                       (lon - truth[:, 1]) * 111_000.0 * np.cos(np.radians(truth[:, 0])))
    use = straight & ~case["planted"]
    use[:8] = False                                                        # the filter is still finding the speed
    raw = float(np.sqrt(np.mean(metres(case["fixes"]["latitude"], case["fixes"]["longitude"])[use] ** 2)))
    filt = float(np.sqrt(np.mean(metres(fr["latitude"], fr["longitude"])[use] ** 2)))
    # the speed: walk again, keeping every record
    c, a, speeds = M.config(**case["cfg"]), M.empty(), []
    for k in range(len(case["icaos"])):
        a, _ = M.step(c, a, ops[k])
        speeds.append(math.hypot(float(a["v_north"]), float(a["v_east"])) if int(a["flags"]) & M.VELOCITY else math.nan)
    speeds, t = np.array(speeds), K.times(case)
    first = float(speeds[np.nonzero(~np.isnan(speeds))[0][0]])
    late = speeds[t > t[-1] - 60.0]
    dflt = run(dict(case, cfg={}))[1]["flags"]
    with capsys.disabled():
        print(f"\nflight with the default accel_h: {int(((dflt & M.OUTLIER) != 0)[~case['planted']].sum())} honest fixes "
              f"gated out in the turn, {int(((dflt & M.RESET) != 0).sum())} restarts")
        print(f"flight: {len(t)} fixes, {int(case['planted'].sum())} displaced; straight legs RMS raw {raw:.1f} m, "
              f"filtered {filt:.1f} m, ratio {filt / raw:.2f}; speed at min_run {first:.1f} m/s, last 60 s RMS error "
              f"{float(np.sqrt(np.mean((late - 230.0) ** 2))):.1f} m/s")
    assert filt < raw
    phys = D.filter_physical(np.array([state[int(case["icaos"][0])]]).view(A.AIRCRAFT_FILTER_DTYPE))[0]
    assert abs(phys["ground_speed_kt"] - speeds[-1] * 3600.0 / 1852.0) < 1e-9 and 0.0 <= phys["track_deg"] < 360.0
    assert abs(phys["track_deg"] - 130.0) < 5.0 and phys["position_sigma_m"] < 100.0 and abs(phys["vertical_rate_fpm"]) < 600.0
    assert np.isnan(D.filter_physical(D.filter_empty(1))[0]["ground_speed_kt"])
