"""Clock sync on the CPU mirror (adsb_host_clock_sync, adsb_host_clock_apply) against the independent numpy model of
tests/clock_model.py and against the truth of the scenarios in tests/clock_cases.py.  The helpers here take the
implementation as a pair of functions, so tests/test_gpu_clock.py runs the same checks on the device."""
import ctypes as C

import numpy as np
import pytest

import air_rs_amd as A
from tests import clock_cases as CC
from tests import clock_model as CM
from tests import mlat_model as M


def mirror_sync(rcv, lst, **cfg):
    return A.host_clock_sync(rcv, lst["msgs"], lst["recs"], lst["rx"], **cfg)


def model_sync(rcv, lst, **cfg):
    return CM.clock_sync(rcv, lst["msgs"], lst["recs"], lst["rx"], **cfg)


def same_clocks(got, gh, want, wh, prior, tol_s, tol_drift, name):
    """Integer fields equal, fine offsets and drifts within the tolerances, offset_s = prior + fine_offset_s to the bit
    (its definition) -> (largest offset gap, largest drift gap)."""
    for k in CM.INTEGER_FIELDS:
        assert (got[k] == want[k]).all(), (name, k, got[k], want[k])
    for k in ("n_messages", "n_eligible", "n_rows", "n_dropped", "n_reached", "flags"):
        assert int(gh[k]) == int(wh[k]), (name, k, int(gh[k]), int(wh[k]))
    assert (got["reserved"] == 0).all()
    da = float(np.abs(got["fine_offset_s"] - want["fine_offset_s"]).max())
    db = float(np.abs(got["drift"] - want["drift"]).max())
    assert da <= tol_s and db <= tol_drift, (name, da, db)
    assert (got["offset_s"] == np.asarray(prior, dtype=np.float64) + got["fine_offset_s"]).all(), name
    # residual_rms_s is a float of a closed form over the pair sums, whose six terms are each about n x y'^2 and carry a
    # few roundings each: the squared sum is off by about 24 x 2.2e-16 x n x max(y'^2), the rms by sqrt(24 x 2.2e-16) =
    # 7.3e-8 of the largest |y'|, which in these scenarios (offsets 1e-3 s, drifts 1e-4 over 60 s, both ends) stays
    # under 1e-2 s: 7.3e-10 s absolute, beside 1e-3 relative for the float and the order of the sums
    assert np.allclose(got["residual_rms_s"], want["residual_rms_s"], rtol=1e-3, atol=7.3e-10), name
    return da, db


@pytest.fixture(scope="module")
def cases(oracle):
    return CC.case_lists(oracle)


def test_mirror_equals_model(lib, cases):
    worst = [0.0, 0.0]
    for name, sc, kw in cases:
        cfg = dict(sc["cfg"], **kw)
        got, gh, state = A.host_clock_sync(sc["rcv"], sc["lst"]["msgs"], sc["lst"]["recs"], sc["lst"]["rx"],
                                           row_state=True, **cfg)
        want, wh, ws, _ = model_sync(sc["rcv"], sc["lst"], **cfg)
        da, db = same_clocks(got, gh, want, wh, sc["rcv"]["clock_offset_s"], CM.MIRROR_VS_MODEL_TOL_S, CM.MIRROR_VS_MODEL_TOL_DRIFT, name)
        assert (state == ws).all(), name
        worst = [max(worst[0], da), max(worst[1], db)]
    print(f"largest mirror-vs-model gap: offset {worst[0]:.3g} s (measured {CM.MIRROR_VS_MODEL_MEASURED_S:.3g}, "
          f"tolerance {CM.MIRROR_VS_MODEL_TOL_S:.3g}), drift {worst[1]:.3g} (measured "
          f"{CM.MIRROR_VS_MODEL_MEASURED_DRIFT:.3g}, tolerance {CM.MIRROR_VS_MODEL_TOL_DRIFT:.3g})")


def check_polar(sync, oracle, reference_sync, tol_s, tol_drift, what):
    """clock_cases.polar: the single-message decode at sites and targets either side of the antimeridian and of the
    87-degree transition.  The counts are the exact reference's (tests/fix_cases.py), the clocks the reference
    implementation's under the given constants -> (largest offset gap, largest drift gap)."""
    sc = CC.polar(oracle)
    lons, lats = sc["rcv"]["longitude"], [np.degrees(M.geodetic_of(p)[2]) for p in sc["pos"]]
    assert (lons > 170).any() and (lons < -170).any() and min(lats) < 87 < max(lats)
    eligible, rows = CC.exact_counts(sc)
    assert eligible > 100 and rows > 300
    got, gh = sync(sc["rcv"], sc["lst"], **sc["cfg"])[:2]
    want, wh = reference_sync(sc["rcv"], sc["lst"], **sc["cfg"])[:2]
    assert (int(gh["n_eligible"]), int(gh["n_rows"])) == (int(wh["n_eligible"]), int(wh["n_rows"])) == (eligible, rows)
    da, db = same_clocks(got, gh, want, wh, sc["rcv"]["clock_offset_s"], tol_s, tol_drift, what)
    print(f"polar scenario, {what}: gap {da:.3g} s, {db:.3g} s/s; {eligible} eligible messages, {rows} rows")
    return da, db


def test_polar_antimeridian_scenario(lib, oracle):
    check_polar(mirror_sync, oracle, model_sync, CM.MIRROR_VS_MODEL_TOL_S, CM.MIRROR_VS_MODEL_TOL_DRIFT, "mirror vs model")
    sc = CC.polar(oracle)
    ta, tb = CC.truth(sc)
    got = mirror_sync(sc["rcv"], sc["lst"], **sc["cfg"])[0]
    assert np.abs(got["fine_offset_s"] - ta).max() < 2e-7 and np.abs(got["drift"] - tb).max() < 2e-8   # as check_truth's


TRUTH_ROWS = (("6 receivers, 12 MHz ticks", dict(n_rcv=6, n_msgs=300, seed=21)),
              ("8 receivers, 2 MHz samples", dict(n_rcv=8, n_msgs=300, seed=22, spt=0.5e-6)),
              ("33 receivers, heard 0.3, 20 s", dict(n_rcv=33, n_msgs=300, seed=23, p_heard=0.3, span_s=20.0)))


def check_truth(sync, oracle, name):
    """The implementation's error against the scenario's true clocks is at most twice the model's own."""
    sc = CC.scenario(oracle, **dict(TRUTH_ROWS)[name])
    ta, tb = CC.truth(sc)
    want = model_sync(sc["rcv"], sc["lst"], **sc["cfg"])[0]
    ea, eb = np.abs(want["fine_offset_s"] - ta).max(), np.abs(want["drift"] - tb).max()
    got = sync(sc["rcv"], sc["lst"], **sc["cfg"])[0]
    ga, gb = np.abs(got["fine_offset_s"] - ta).max(), np.abs(got["drift"] - tb).max()
    print(f"{name}: model error {ea:.3g} s, {eb:.3g} s/s; implementation {ga:.3g} s, {gb:.3g} s/s")
    assert (got["flags"] & CM.REACHED).all() and ga <= 2 * ea and gb <= 2 * eb, (name, ga, ea, gb, eb)
    assert ea < 2e-7 and eb < 2e-8          # the scenario itself is sound: the issue's experiment found 1.6e-8 .. 3.6e-8


@pytest.mark.parametrize("name", [r[0] for r in TRUTH_ROWS])
def test_truth(lib, oracle, name):
    check_truth(mirror_sync, oracle, name)


OUTLIER_LIMIT_S = 1e-6


def check_outliers(sync, oracle, row_state=None):
    """Seed 11: checked on the CPU that no residual of the model's first pass lies within 1e-9 s of the 1e-6 s limit
    (asserted below).  Every dropped row belongs to a planted message, the dropped counts equal the model's, and the
    second pass is closer to the truth than the first."""
    sc, planted = CC.outliers(oracle)
    cfg = dict(sc["cfg"], max_residual_s=OUTLIER_LIMIT_S)
    want, wh, ws, first_residual = model_sync(sc["rcv"], sc["lst"], **cfg)
    assert min(abs(abs(v) - OUTLIER_LIMIT_S) for v in first_residual.values()) > 1e-9
    msg_of = np.repeat(np.arange(len(sc["lst"]["msgs"])), sc["lst"]["msgs"]["n_receptions"])
    assert wh["n_dropped"] > 0 and set(msg_of[ws == 2].tolist()) <= planted
    ta, _ = CC.truth(sc)
    one = sync(sc["rcv"], sc["lst"], **sc["cfg"])[0]
    got, gh = sync(sc["rcv"], sc["lst"], **cfg)[:2]
    e1, e2 = np.abs(one["fine_offset_s"] - ta).max(), np.abs(got["fine_offset_s"] - ta).max()
    em = np.abs(want["fine_offset_s"] - ta).max()
    print(f"outliers: first pass off by {e1:.3g} s, second by {e2:.3g} s (model {em:.3g} s) after dropping "
          f"{int(gh['n_dropped'])} of {int(gh['n_rows'])} rows")
    same_clocks(got, gh, want, wh, sc["rcv"]["clock_offset_s"], CM.MIRROR_VS_MODEL_TOL_S, CM.MIRROR_VS_MODEL_TOL_DRIFT, "outliers")
    assert e2 <= 2 * em and e2 < e1
    if row_state is not None:
        assert (row_state(sc["rcv"], sc["lst"], **cfg) == ws).all()


def test_outliers(lib, oracle):
    check_outliers(mirror_sync, oracle,
                   lambda rcv, lst, **cfg: A.host_clock_sync(rcv, lst["msgs"], lst["recs"], lst["rx"], row_state=True,
                                                             **cfg)[2])


def shape_lists(oracle, per_block=16):
    """(name, scenario, sync keywords, expectations) at the smallest shapes at which each path can go wrong."""
    out = []
    add = lambda name, sc, kw=None, **expect: out.append((name, sc, kw or {}, expect))
    sc = CC.scenario(oracle, 3, 0, seed=30)
    sc["cfg"] = dict(time_source="reception", seconds_per_tick=CC.SPT_12MHZ)      # ticks would need rx records
    add("no message", sc, n_rows=0, reached=[0])
    add("one receiver", CC.scenario(oracle, 1, 3, seed=29), n_rows=0, reached=[0])
    add("one message", CC.scenario(oracle, 4, 1, seed=31, p_heard=1.0), hdr_flags=CM.HDR_DRIFT_DROPPED)
    for n in (per_block - 1, per_block, per_block + 1):
        add(f"{n} messages", CC.scenario(oracle, 6, n, seed=32 + n))
    sc = CC.scenario(oracle, 5, 12, seed=40, p_heard=1.0, times=[3.0] * 12, drift=0.0)
    sc["lst"]["msgs"]["time"][:] = sc["lst"]["msgs"]["time"][0]                    # one tau: no drift can be told
    add("all messages at one time", sc, hdr_flags=CM.HDR_DRIFT_DROPPED)
    # pair segments of 1, 63, 64, 65 and 200 rows: two receivers that both hear every message
    for n in (1, 63, 64, 65, 200):
        add(f"segment of {n}", CC.scenario(oracle, 2, n, seed=50 + n, p_heard=1.0), n_rows=n)
    heard = [[0, 1]] * 150 + [[0, 2 + i] for i in range(30)]
    add("one pair with 150 rows, 30 with one", CC.scenario(oracle, 32, 180, seed=60, heard=heard), dict(drift=False),
        n_rows=180, partners=[31] + [1] * 31)
    # reached set
    add("a receiver nobody shares a message with", CC.scenario(oracle, 4, 30, seed=61, heard=[[0, 1, 2]] * 29 + [[3]]),
        reached=[0, 1, 2])
    chain = [[0, 1], [1, 2], [2, 3]] * 12
    add("chain 0-1-2-3", CC.scenario(oracle, 4, 36, seed=62, heard=chain), reached=[0, 1, 2, 3], partners=[1, 2, 2, 1])
    add("min_rows cuts the chain", CC.scenario(oracle, 4, 36, seed=62, heard=chain[:-1] + [[0, 1]]),
        dict(min_rows=12), reached=[0, 1, 2])
    add("reference 2", CC.scenario(oracle, 5, 40, seed=63), dict(reference=2))
    add("offsets only", CC.scenario(oracle, 5, 40, seed=64, drift=0.0), dict(drift=False))
    # times
    add("ticks wrap 2^48", CC.scenario(oracle, 4, 40, seed=65, tick_base=(1 << 48) - 12_000_000 * 20, mod48=True))
    sc = CC.scenario(oracle, 4, 40, seed=66, offset_s=np.array([0.0, 1000.0, -1000.0, 3.25e-4]), tick_base=30_000_000_000,
                     p_heard=1.0)    # everyone hears everything: the message times are all on receiver 2's clock
    sc["rcv"]["clock_offset_s"] = [0.0, 1000.0, -1000.0, 0.0]
    add("priors of +-1000 s", sc)
    sc = CC.scenario(oracle, 4, 40, seed=67, tick_base=(1 << 53) + 12345)
    sc["cfg"] = dict(time_source="reception", seconds_per_tick=CC.SPT_12MHZ)
    add("reception times above 2^53", sc)
    add("256 receivers, two emitters", CC.many_receivers(oracle), n_rows=510)
    # ineligible messages and the used rule
    frames = lambda **kw: (lambda o, pos: CC.position_frames(o, pos, **kw))
    add("TC 19", CC.scenario(oracle, 4, 8, seed=70, frames_of=frames(tc=19)), n_rows=0)
    add("surface", CC.scenario(oracle, 4, 8, seed=71, frames_of=frames(tc=6)), n_rows=0)
    add("Q bit clear", CC.scenario(oracle, 4, 8, seed=72, frames_of=frames(altitude_code=0x3A8 & ~0x10)), n_rows=0)
    add("too far", CC.scenario(oracle, 4, 8, seed=73, p_heard=1.0), dict(max_range_nm=1.0), n_rows=0)
    add("a receiver twice in a message",
        CC.scenario(oracle, 4, 20, seed=74, p_heard=1.0, extra=[(g, g % 4, 5 + g) for g in range(0, 20, 2)]), n_rows=60)
    return out


def check_shape(sync, name, sc, kw, expect, tol_s, tol_drift, reference_sync=model_sync):
    cfg = dict(sc["cfg"], **kw)
    want, wh = reference_sync(sc["rcv"], sc["lst"], **cfg)[:2]
    got, gh = sync(sc["rcv"], sc["lst"], **cfg)[:2]
    da, db = same_clocks(got, gh, want, wh, sc["rcv"]["clock_offset_s"], tol_s, tol_drift, name)
    print(f"{name}: gap {da:.3g} s, {db:.3g} s/s")
    if "n_rows" in expect:
        assert int(gh["n_rows"]) == expect["n_rows"], name
    if "hdr_flags" in expect:
        assert int(gh["flags"]) == expect["hdr_flags"] and (got["drift"] == 0).all(), name
    if "reached" in expect:
        assert np.flatnonzero(got["flags"] & CM.REACHED).tolist() == expect["reached"], name
        out = (got["flags"] & CM.REACHED) == 0
        assert (got["fine_offset_s"][out] == 0).all() and (got["drift"][out] == 0).all(), name
    if "partners" in expect:
        assert got["n_partners"].tolist() == expect["partners"], name
    ref = kw.get("reference", 0)
    assert got["flags"][ref] & CM.REFERENCE and got["fine_offset_s"][ref] == 0 and got["drift"][ref] == 0
    return got, gh


def test_shapes(lib, oracle):
    for name, sc, kw, expect in shape_lists(oracle):
        got, gh = check_shape(mirror_sync, name, sc, kw, expect, CM.MIRROR_VS_MODEL_TOL_S, CM.MIRROR_VS_MODEL_TOL_DRIFT)
        if name in ("priors of +-1000 s", "ticks wrap 2^48", "reception times above 2^53", "chain 0-1-2-3", "reference 2"):
            ta, tb = CC.truth(sc, kw.get("reference", 0))
            assert np.abs(got["fine_offset_s"] - ta).max() < 5e-7, (name, got["fine_offset_s"], ta)


def bad_index_lists(oracle):
    """(name, receivers, list) with one message that names something the lists do not have."""
    sc = CC.scenario(oracle, 4, 20, seed=80, p_heard=1.0)
    lst = sc["lst"]
    out = []
    a = {k: v.copy() for k, v in lst.items()}
    a["recs"]["receiver"][int(a["msgs"]["first"][5]) + 2] = 4                       # a receiver >= R
    out.append(("receiver >= R", sc, a))
    b = {k: v.copy() for k, v in lst.items()}
    b["msgs"]["n_receptions"][19] += 1                                             # receptions past recs[N]
    out.append(("receptions past the list", sc, b))
    c = {k: v.copy() for k, v in lst.items()}
    c["recs"]["frame"][int(c["msgs"]["first"][7]) + 1] = len(c["rx"])              # a frame >= n_rx
    out.append(("frame >= n_rx", sc, c))
    return out


def test_bad_index(lib, oracle):
    for name, sc, lst in bad_index_lists(oracle):
        want, wh = model_sync(sc["rcv"], lst, **sc["cfg"])[:2]
        c = A.demod._clock_cfg(**sc["cfg"])
        clocks, hdr = np.zeros(4, dtype=A.CLOCK_DTYPE), A._lib.AdsbClockHeader()
        rc = A.load().adsb_host_clock_sync(C.byref(c), sc["rcv"].ctypes.data, 4, lst["msgs"].ctypes.data, len(lst["msgs"]),
                                           lst["recs"].ctypes.data, len(lst["recs"]), lst["rx"].ctypes.data, len(lst["rx"]),
                                           clocks.ctypes.data, C.byref(hdr), None)
        assert rc == A.ADSB_E_ARG and hdr.flags == CM.HDR_BAD_INDEX == wh["flags"], name
        assert hdr.n_eligible == wh["n_eligible"] == 19 and hdr.n_rows == wh["n_rows"] == 57, name
        assert np.abs(clocks["fine_offset_s"] - want["fine_offset_s"]).max() <= CM.MIRROR_VS_MODEL_TOL_S, name


APPLY_HALF = 1e-3


def check_apply(corrected, sc, clocks, name):
    """Corrected times against the model's: equal, or one unit apart where the model's llrint argument lies within 1e-3
    of a half -> how many receptions that excuses (at most 1 % of the list)."""
    lst = sc["lst"]
    want, half = CM.apply(clocks, lst["msgs"], lst["recs"], lst["rx"], **sc["cfg"])
    assert (corrected["frame"] == lst["recs"]["frame"]).all() and (corrected["receiver"] == lst["recs"]["receiver"]).all()
    assert (corrected["reserved"] == 0).all()
    gap = (corrected["time"] - want["time"]).astype(np.int64)
    near = half < APPLY_HALF
    assert (gap[~near] == 0).all() and (np.abs(gap[near]) <= 1).all(), name
    left_out = int((gap != 0).sum())
    assert left_out <= len(gap) // 100, (name, left_out)
    return left_out


def test_apply(lib, oracle, cases):
    total = 0
    for name, sc, kw in cases:
        lst, cfg = sc["lst"], dict(sc["cfg"], **kw)
        clocks = mirror_sync(sc["rcv"], lst, **cfg)[0]
        corrected = A.host_clock_apply(clocks, lst["msgs"], lst["recs"], lst["rx"], **sc["cfg"])
        total += check_apply(corrected, sc, clocks, name)
    print(f"receptions left out for a llrint argument within {APPLY_HALF} of a half: {total}")


def end_to_end_list(oracle):
    """The "12 MHz ticks, offsets, partial" style of list with drifts, every second message a TC 19 frame."""
    def frames(o, pos):
        out = CC.position_frames(o, pos)
        return [CC.position_frames(o, pos[i:i + 1], tc=19)[0] if i % 2 else f for i, f in enumerate(out)]
    # 5 to 9 receivers per message: with 4 and no altitude (the TC 19 half) the solver's two solutions are both VALID even
    # on perfect clocks (one of 129 such fixes was 51 km off on this list with all offsets and drifts 0)
    rng = np.random.default_rng(90)
    heard = [sorted(rng.choice(9, size=int(rng.integers(5, 10)), replace=False).tolist()) for _ in range(240)]
    sc = CC.scenario(oracle, 9, 240, seed=90, heard=heard, frames_of=frames)
    sc["rcv"]["clock_offset_s"] = np.round(sc["offsets"] * 1e4) / 1e4              # priors good to 50 us
    return sc


def check_end_to_end(sc, clocks, corrected, solve, clock_bound_s):
    """The existing solver on the raw list with the priors against the same solver on the corrected receptions."""
    lst = sc["lst"]
    raw, _ = solve(sc["rcv"], lst["msgs"], lst["recs"], lst["rx"], time_source="ticks", use_altitude=True)
    plain = sc["rcv"].copy()
    plain["clock_offset_s"] = 0.0
    fixed, _ = solve(plain, lst["msgs"], corrected, None, seconds_per_tick=sc["spt"] / 256, use_altitude=True)

    def errors(fixes):
        return np.array([np.sqrt(((M.ecef_of(f["latitude"], f["longitude"], f["height_m"]) - p) ** 2).sum())
                         for f, p in zip(fixes, sc["pos"])])
    good = lambda fixes: int(((fixes["flags"] & M.VALID != 0) & (errors(fixes) < 100.0)).sum())
    n_raw, n_fixed = good(raw), good(fixed)
    print(f"end to end: {n_raw} VALID fixes under 100 m on the raw list, {n_fixed} on the corrected one, of {len(raw)}")
    assert n_raw < n_fixed
    # tests/test_gpu_mlat.py's bound against the true positions, 3 x a tick's range x the largest pdop (a tick of
    # 1 / 12e6 s is 25 m), with c x the clock bound added to the range
    sel = (fixed["flags"] & M.VALID != 0) & (fixed["pdop"] <= 20)
    bound = (M.C_AIR * sc["spt"] * 3 + M.C_AIR * clock_bound_s) * fixed["pdop"][sel].max()
    assert sel.sum() >= 50 and errors(fixed)[sel].max() < bound, (errors(fixed)[sel].max(), bound)


def test_end_to_end(lib, oracle):
    sc = end_to_end_list(oracle)
    lst = sc["lst"]
    clocks = mirror_sync(sc["rcv"], lst, **sc["cfg"])[0]
    ta, _ = CC.truth(sc)
    model = model_sync(sc["rcv"], lst, **sc["cfg"])[0]
    corrected = A.host_clock_apply(clocks, lst["msgs"], lst["recs"], lst["rx"], **sc["cfg"])
    check_end_to_end(sc, clocks, corrected, A.host_multilaterate, 2 * np.abs(model["fine_offset_s"] - ta).max())
