"""adsb_host_multilaterate, the CPU mirror of the device's multilaterate, against the independent numpy model
(tests/mlat_model.py) on the lists of tests/mlat_cases.py, against the truth the lists were built from, and on small
hand-made edge lists with literal expectations (CPU tier)."""
import numpy as np
import pytest

from tests import mlat_cases as K
from tests import mlat_model as M


def same_fixes(got, want, lasts, tol_step, name, tol_m=M.MIRROR_VS_MODEL_TOL_M, gaps=None):
    """The comparison rule of mirror vs model and of device vs mirror: every integer field of every fix agrees, but a
    message whose last step length lies within a factor 10 of the step tolerance may differ in CONVERGED (VALID with
    it) and iterations, at most 1 % of the list; positions of fixes with pdop <= 20 agree within tol_m, and so do their
    hdop, vdop, time_s, height_m and residual_rms_m within the tolerances of M.gaps_of.  A SINGULAR fix has zero
    dilutions; a fix that was not attempted is the same bytes.  Returns the largest position gap found; gaps (a dict)
    takes the largest gap per field."""
    assert len(got) == len(want), name
    left_out, worst = 0, 0.0
    gaps = {} if gaps is None else gaps
    for g, (a, b) in enumerate(zip(got, want)):
        ints = lambda f: (int(f["flags"]), int(f["n_used"]), int(f["iterations"]))
        if ints(a) != ints(b):
            near = lasts is not None and tol_step / 10 < lasts[g] < tol_step * 10
            loose = M.CONVERGED | M.VALID
            assert near and a["n_used"] == b["n_used"] and int(a["flags"]) & ~loose == int(b["flags"]) & ~loose, \
                (name, g, ints(a), ints(b))
            left_out += 1
            continue
        if a["flags"] & M.ATTEMPTED and not a["flags"] & M.SINGULAR and b["pdop"] <= 20:
            gap = M.position_gap_m(a, b)
            worst = max(worst, gap)
            assert gap <= tol_m, (name, g, gap)
            assert abs(float(a["pdop"]) - float(b["pdop"])) <= 1e-3 * float(b["pdop"]), (name, g)
            for field, (gap, tol) in M.gaps_of(a, b).items():
                gaps[field] = max(gaps.get(field, 0.0), gap)
                assert gap <= tol, (name, g, field, gap, tol, a[field], b[field])
        if a["flags"] & M.SINGULAR:
            assert a["pdop"] == 0 and a["hdop"] == 0 and a["vdop"] == 0, (name, g)
        if not a["flags"] & M.ATTEMPTED:
            assert a.tobytes() == b.tobytes(), (name, g)
    assert left_out <= len(want) / 100, (name, left_out)
    return worst


@pytest.fixture(scope="module")
def cases(oracle):
    """(name, receivers, list, cfg, the model's fixes, the model's last step lengths) per case list, computed once."""
    return [(name, rcv, lst, cfg, want, lasts) for name, rcv, lst, cfg, expect, want, _, lasts in K.modelled(oracle)
            if expect is None]


def _say(what, gaps):
    print(f"largest {what} gaps over fixes with pdop <= 20: " + ", ".join(
        f"{k} {gaps.get(k, 0.0):.3g} (recorded {M.MIRROR_VS_MODEL_MEASURED[k]:.3g}, tolerance {tol:.3g})"
        for k, tol in M.MIRROR_VS_MODEL_TOL.items()))


def test_mirror_equals_model(lib, cases):
    worst, gaps = 0.0, {}
    for name, rcv, lst, cfg, want, lasts in cases:
        got, hdr = lib.host_multilaterate(rcv, lst["msgs"], lst["recs"], lst["rx"], **cfg)
        worst = max(worst, same_fixes(got, want, lasts, 0.01, name, gaps=gaps))
        assert int(hdr["n_messages"]) == len(want) and int(hdr["flags"]) == 0
        assert int(hdr["n_attempted"]) == int((got["flags"] & M.ATTEMPTED != 0).sum())
        assert int(hdr["n_valid"]) == int((got["flags"] & M.VALID != 0).sum())
    print(f"largest mirror-vs-model position gap over fixes with pdop <= 20: {worst:.3g} m "
          f"(recorded {M.MIRROR_VS_MODEL_MEASURED_M:.3g} m, tolerance {M.MIRROR_VS_MODEL_TOL_M:.3g} m)")
    _say("mirror-vs-model", gaps)


def test_edge_lists_mirror_equals_model(lib, oracle):
    """The edge lists of tests/mlat_cases.py: the mirror against the model under same_fixes with NO message left out,
    and both held to the lists' literal expectations.  The measured gaps, over the case lists too, are the recorded
    ones (tests/mlat_model.py, profiles/mlat_edges_checks.txt)."""
    worst, gaps, of_mirror, of_model = 0.0, {}, {}, {}
    for name, rcv, lst, cfg, expect, want, want_hdr, lasts in K.modelled(oracle):
        got, hdr = lib.host_multilaterate(rcv, lst["msgs"], lst["recs"], lst["rx"], **cfg)
        tol = cfg.get("step_tol_m") or 0.01
        worst = max(worst, same_fixes(got, want, lasts, tol, name, gaps=gaps))
        if expect is None:
            continue
        assert len(want) <= 32 and [ints for ints in zip(got["flags"], got["n_used"], got["iterations"])] == \
            [ints for ints in zip(want["flags"], want["n_used"], want["iterations"])], name
        of_model[name], of_mirror[name] = want, got
        error = K.check_expectations(name, want, want_hdr, expect, of_model, lasts, tol)
        mine = K.check_expectations(name, got, hdr, expect, of_mirror, lasts, tol, model_error=error)
        if error is not None:
            print(f"{name}: largest error against the truth, model {error:.2f} m, mirror {mine:.2f} m")
    print(f"largest mirror-vs-model position gap, case and edge lists: {worst:.3g} m")
    _say("mirror-vs-model (case and edge lists)", gaps)
    assert worst <= M.MIRROR_VS_MODEL_MEASURED_M * 1.005
    for k, v in gaps.items():
        assert v <= M.MIRROR_VS_MODEL_MEASURED[k], (k, v)


def test_recorded_figures_are_the_profile_s():
    """The constants of tests/mlat_model.py and tests/mlat_exact.py equal what profiles/mlat_edges_checks.txt records."""
    import os
    import re
    from tests import mlat_exact as X
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                             "mlat_edges_checks.txt")).read()
    said = {k: float(v) for k, v in re.findall(r"^\s+recorded (\S+) = (\S+)$", text, flags=re.M)}
    want = {f"mirror_vs_model.{k}": v for k, v in M.MIRROR_VS_MODEL_MEASURED.items()}
    want.update({f"exact_on_model.{k}": v for k, v in X.MODEL_MEASURED.items()})
    want["mirror_vs_model.position_m"] = M.MIRROR_VS_MODEL_MEASURED_M
    want["rms_floor_m"] = float(f"{M.RMS_FLOOR_M:.3g}")
    assert said == want


def test_case_lists_cover_the_shapes(cases):
    """What the comparisons above rest on: attempted and not attempted messages, both stages, altitude and none,
    several receptions per partial sum."""
    flags = np.concatenate([c[4]["flags"] for c in cases])
    used = np.concatenate([c[4]["n_used"] for c in cases])
    assert (flags & M.TOO_FEW).any() and (flags & M.VALID).any() and (flags & M.ALTITUDE).any()
    assert {3, 4, 16, 17, 33} <= set(used.tolist())
    by = {c[0]: c for c in cases}
    _, _, lst, _, want, _ = by["repeated receivers"]
    twice = lst["msgs"]["n_receptions"] == 8
    assert twice.sum() == 10 and (want["n_used"] == 7).all()       # the later reception of a receiver is not used


@pytest.mark.parametrize("row", K.TRUTH_ROWS, ids=[r[0] for r in K.TRUTH_ROWS])
def test_truth(lib, oracle, row):
    """At 1 ns ticks at least 99 % of the messages are VALID and every valid fix lies within 3 x the numpy experiment's
    largest error for its row (20.6 m, 15.7 m, 15.7 m).  The model on this generator gave 28.9 m, 16.9 m and 13.5 m
    (profiles/mlat_checks.txt)."""
    rcv, lst, cfg, pos, err = K.truth_list(oracle, row[0])
    got, hdr = lib.host_multilaterate(rcv, lst["msgs"], lst["recs"], **cfg)
    valid = got["flags"] & M.VALID != 0
    assert valid.sum() >= 0.99 * len(got) and int(hdr["n_valid"]) == valid.sum()
    assert ((got["flags"] & M.ALTITUDE != 0) == cfg["use_altitude"]).all()
    gaps = [float(np.sqrt(((M.ecef_of(f["latitude"], f["longitude"], f["height_m"]) - p) ** 2).sum()))
            for f, p in zip(got[valid], pos[valid])]
    print(f"{row[0]}: {valid.sum()} of {len(got)} valid, largest 3-D error {max(gaps):.2f} m, bound {3 * err:.1f} m")
    assert max(gaps) <= 3 * err


# ---- edges: literal expectations on small hand-made lists ----

def _small(oracle, n_rcv, n_em=3, seed=0, **kw):
    rcv = K.receivers(n_rcv, seed=700 + n_rcv + seed)
    pos, frames = K.emitters(oracle, n_em, seed=800 + n_rcv + seed)
    return rcv, pos, frames, K.build(rcv, pos, frames, **kw)


def test_used_rule(lib, oracle):
    rcv, pos, frames, plain = _small(oracle, 6)
    twice = K.build(rcv, pos, frames, extra=[(0, 2, 25), (1, 0, 1), (2, 5, 300)])
    a, _ = lib.host_multilaterate(rcv, plain["msgs"], plain["recs"], seconds_per_tick=K.SPT_NS)
    b, _ = lib.host_multilaterate(rcv, twice["msgs"], twice["recs"], seconds_per_tick=K.SPT_NS)
    assert twice["msgs"]["n_receptions"].tolist() == [7, 7, 7] and b["n_used"].tolist() == [6, 6, 6]
    assert (a["flags"] == b["flags"]).all() and (a["flags"] & M.VALID).all()
    # the later reception is ignored: the same fix (other partial sums hold the rows, so not the same bits)
    assert max(M.position_gap_m(x, y) for x, y in zip(a, b)) <= M.MIRROR_VS_MODEL_TOL_M


def test_too_few_and_the_altitude_floor(lib, oracle):
    rcv, _, _, lst = _small(oracle, 3)
    free, hf = lib.host_multilaterate(rcv, lst["msgs"], lst["recs"], seconds_per_tick=K.SPT_NS)
    assert (free["flags"] == M.TOO_FEW).all() and (free["n_used"] == 3).all() and int(hf["n_attempted"]) == 0
    for f in free:
        assert f.tobytes()[:48] == bytes(48) and f["iterations"] == 0      # zero position fields
    alt, ha = lib.host_multilaterate(rcv, lst["msgs"], lst["recs"], seconds_per_tick=K.SPT_NS, use_altitude=True)
    assert (alt["flags"] & (M.ATTEMPTED | M.ALTITUDE) == M.ATTEMPTED | M.ALTITUDE).all() and int(ha["n_attempted"]) == 3
    more, _ = lib.host_multilaterate(rcv, lst["msgs"], lst["recs"], seconds_per_tick=K.SPT_NS, use_altitude=True,
                                     min_receivers=4)
    assert (more["flags"] == M.TOO_FEW).all()


def test_too_many(lib, oracle):
    rcv = K.receivers(256, seed=756)
    pos, frames = K.emitters(oracle, 2, seed=856)
    lst = K.build(rcv, pos, frames, extra=[(0, 5, 10)])
    assert lst["msgs"]["n_receptions"].tolist() == [257, 256]
    got, hdr = lib.host_multilaterate(rcv, lst["msgs"], lst["recs"], seconds_per_tick=K.SPT_NS)
    assert got["flags"][0] == M.TOO_MANY and got[0].tobytes()[:52] == bytes(52)
    assert got["flags"][1] & M.VALID and got["n_used"][1] == 256
    assert (int(hdr["n_messages"]), int(hdr["n_attempted"]), int(hdr["n_valid"])) == (2, 1, 1)


def test_all_stations_equal_is_singular(lib, oracle):
    rcv, pos, frames, _ = _small(oracle, 5)
    rcv[:] = rcv[0]
    lst = K.build(rcv, pos, frames)
    for alt in (False, True):
        got, hdr = lib.host_multilaterate(rcv, lst["msgs"], lst["recs"], seconds_per_tick=K.SPT_NS, use_altitude=alt)
        assert (got["flags"] & M.SINGULAR != 0).all() and (got["flags"] & M.VALID == 0).all() and int(hdr["n_valid"]) == 0
        assert (got["pdop"] == 0).all()


def test_tick_wrap(lib, oracle):
    rcv, pos, frames, _ = _small(oracle, 6, n_em=8)
    a = K.build(rcv, pos, frames, spt=1 / 12e6, tick_base=1000)
    b = K.build(rcv, pos, frames, spt=1 / 12e6, tick_base=(1 << 48) - 100_000, mod48=True)
    assert 0 < (b["rx"]["ticks"] < (1 << 47)).sum() < len(b["rx"])          # the list straddles 2^48
    ga, _ = lib.host_multilaterate(rcv, a["msgs"], a["recs"], a["rx"], time_source="ticks")
    gb, _ = lib.host_multilaterate(rcv, b["msgs"], b["recs"], b["rx"], time_source="ticks")
    assert (ga["flags"] & M.VALID).all() and ga.tobytes() == gb.tobytes()


def test_declared_clock_offsets(lib, oracle):
    rcv, pos, frames, plain = _small(oracle, 6, n_em=8)
    ticks = np.array([1, -1, 1, -1, 1, -1]) * 1_000_000                     # +-1 ms at 1 ns ticks
    off = rcv.copy()
    off["clock_offset_s"] = ticks * K.SPT_NS
    shifted = K.build(rcv, pos, frames, offset_ticks=ticks)
    a, _ = lib.host_multilaterate(rcv, plain["msgs"], plain["recs"], seconds_per_tick=K.SPT_NS)
    b, _ = lib.host_multilaterate(off, shifted["msgs"], shifted["recs"], seconds_per_tick=K.SPT_NS)
    c, _ = lib.host_multilaterate(rcv, shifted["msgs"], shifted["recs"], seconds_per_tick=K.SPT_NS)   # not declared
    assert (a["flags"] & M.VALID).all() and (a["flags"] == b["flags"]).all()
    assert max(M.position_gap_m(x, y) for x, y in zip(a, b)) <= M.MIRROR_VS_MODEL_TOL_M
    assert min(M.position_gap_m(x, y) for x, y in zip(a, c)) > 1000.0


def test_rejections(lib, oracle):
    rcv, pos, frames, lst = _small(oracle, 6, n_em=8)
    ok, _ = lib.host_multilaterate(rcv, lst["msgs"], lst["recs"], seconds_per_tick=K.SPT_NS)
    assert (ok["flags"] & M.VALID).all() and (ok["residual_rms_m"] > 1e-6).all()
    res, h = lib.host_multilaterate(rcv, lst["msgs"], lst["recs"], seconds_per_tick=K.SPT_NS, max_residual_m=1e-6)
    assert (res["flags"] == (ok["flags"] ^ M.VALID) | M.REJECTED_RESIDUAL).all() and int(h["n_valid"]) == 0
    rng, h = lib.host_multilaterate(rcv, lst["msgs"], lst["recs"], seconds_per_tick=K.SPT_NS, max_range_m=1000.0)
    assert (rng["flags"] == (ok["flags"] ^ M.VALID) | M.REJECTED_RANGE).all() and int(h["n_valid"]) == 0
    assert rng["latitude"].tobytes() == ok["latitude"].tobytes()            # a rejected fix still says where


def test_empty_list(lib, oracle):
    rcv = K.receivers(4, seed=1)
    none = np.zeros(0, dtype=M.MESSAGE_DTYPE), np.zeros(0, dtype=M.RECEPTION_DTYPE)
    got, hdr = lib.host_multilaterate(rcv, *none, seconds_per_tick=K.SPT_NS)
    assert len(got) == 0 and hdr.tobytes() == bytes(32)
    msgs = np.zeros(2, dtype=M.MESSAGE_DTYPE)                               # messages without receptions
    got, hdr = lib.host_multilaterate(rcv, msgs, none[1], seconds_per_tick=K.SPT_NS)
    assert (got["flags"] == M.TOO_FEW).all() and (got["n_used"] == 0).all() and int(hdr["n_messages"]) == 2
