"""tests/mlat_exact.py: on a hand-made exact scene it finds nothing at the true point and names each broken claim (no
library needed); its measured bounds are the numpy model's own; the CPU mirror's VALID fixes keep every claim on the
case lists and the edge lists of tests/mlat_cases.py (CPU tier)."""
import math

import mpmath as mp
import numpy as np
import pytest

from tests import mlat_cases as K
from tests import mlat_exact as X
from tests import mlat_model as M

# ---- the check itself, on a scene with real-valued rho: no ticks, no rounding, no library ----

SITES = ((47.9, 8.1, 400.0), (47.8, 9.3, 900.0), (47.0, 9.2, 1500.0), (46.9, 8.0, 600.0), (47.45, 8.6, 300.0))
TRUE = (47.31, 8.77, 9144.0)
T0 = -2.0 ** -12                                       # time_s, an f64 exactly


def _scene(altitude=False, moved_m=0.0):
    """(stations, rho, the altitude or None, a fix at the true point moved north by moved_m) with rho_k = range_k +
    T0 c exactly, and the fix's dilutions and rms from numpy (f64) at the true point."""
    with mp.workdps(X.DIGITS):
        st = [X.ecef_of(*s) for s in SITES]
        p = X.ecef_of(*TRUE)
        rho = [mp.sqrt(sum((a - b) ** 2 for a, b in zip(p, s))) + mp.mpf(T0) * mp.mpf(M.C_AIR) for s in st]
    P, S = M.ecef_of(*TRUE), np.array([M.ecef_of(*s) for s in SITES])
    d = P - S
    J = np.hstack([d / np.sqrt((d * d).sum(axis=1))[:, None], np.ones((len(S), 1))])
    phi, lam = math.radians(TRUE[0]), math.radians(TRUE[1])
    up = np.array([math.cos(phi) * math.cos(lam), math.cos(phi) * math.sin(lam), math.sin(phi)])
    if altitude:
        J = np.vstack([J, np.append(up, 0.0)])
    Q = np.linalg.inv(J.T @ J)[:3, :3]
    east = np.array([-math.sin(lam), math.cos(lam), 0.0])
    north = np.array([-math.sin(phi) * math.cos(lam), -math.sin(phi) * math.sin(lam), math.cos(phi)])
    fix = np.zeros(1, dtype=M.FIX_DTYPE)[0]
    fix["latitude"], fix["longitude"], fix["height_m"] = TRUE[0] + moved_m / 111200.0, TRUE[1], TRUE[2]
    fix["time_s"], fix["n_used"] = T0, len(SITES)
    fix["pdop"], fix["hdop"], fix["vdop"] = math.sqrt(np.trace(Q)), math.sqrt(east @ Q @ east + north @ Q @ north), \
        math.sqrt(up @ Q @ up)
    fix["flags"] = M.ATTEMPTED | M.CONVERGED | M.VALID | (M.ALTITUDE if altitude else 0)
    return st, rho, (mp.mpf(TRUE[2]) if altitude else None), fix, Q, (east, north, up)


@pytest.mark.parametrize("altitude", [False, True])
def test_nothing_to_find_at_the_true_point(altitude):
    st, rho, alt, fix, _, _ = _scene(altitude)
    fig = X.figures(st, rho, alt, fix)
    assert fig["rows"] == 5 + altitude
    assert fig["rms_exact"] < 1e-30 and fig["step_m"] < 1e-30 and fig["time_s"] < 1e-40
    assert max(fig["pdop"], fig["hdop"], fig["vdop"]) < 1e-7               # numpy's f64 dilutions, stored as f32
    assert X.broken(fig, 5) == []


def test_a_point_one_metre_off_is_one_step_away():
    st, rho, alt, fix, _, _ = _scene(moved_m=1.0)
    fig = X.figures(st, rho, alt, fix)
    assert 0.99 < fig["step_m"] < 1.01 and fig["rms_exact"] > 0.01
    assert {b[0] for b in X.broken(fig, 5)} >= {"step_m", "residual_rms_m"}


def test_each_broken_claim_is_named():
    st, rho, alt, fix, Q, (east, north, up) = _scene(altitude=True)
    def names(**fields):
        f = fix.copy()
        for k, v in fields.items():
            f[k] = v
        return {b[0] for b in X.broken(X.figures(st, rho, alt, f), 5)}
    assert names() == set()
    lam = math.radians(TRUE[1])
    transposed = np.array([-math.cos(lam), math.sin(lam), 0.0])            # sin and cos of the longitude exchanged
    assert names(hdop=math.sqrt(transposed @ Q @ transposed + north @ Q @ north)) == {"hdop"}
    assert names(vdop=math.sqrt(north @ Q @ north)) == {"vdop"}
    assert names(pdop=math.sqrt(Q[0, 0] + Q[1, 1])) == {"pdop"}
    assert names(time_s=T0 * M.C_AIR) >= {"time_s", "residual_rms_m"}      # metres where seconds belong
    assert names(time_s=T0 + 1e-12) >= {"time_s"}                          # 0.3 mm of range
    assert names(residual_rms_m=1e-3) == {"residual_rms_m"}
    # the height identity: 3 receivers and the altitude, 2 rms + the floor
    f = fix.copy()
    f["height_m"], f["residual_rms_m"] = TRUE[2] + 0.5, 0.2
    assert "height_m" in {b[0] for b in X.broken(X.figures(st[:3], rho[:3], alt, f), 3)}
    assert "height_m" not in {b[0] for b in X.broken(X.figures(st[:3], rho[:3], alt, f), 3, valid=False)}


def test_exact_height_and_rho():
    with mp.workdps(X.DIGITS):
        for lat, lon, h in ((89.9999, -179.9, -300.0), (-86.8, 179.8, 15293.0), (0.0, 0.0, 0.0), (47.0, 8.0, 1e5)):
            got_h, phi, lam = X.geodetic_of(X.ecef_of(lat, lon, h))
            assert abs(got_h - mp.mpf(h)) < 1e-35 and abs(phi * 180 / mp.pi - mp.mpf(lat)) < 1e-40
            assert abs(lam * 180 / mp.pi - mp.mpf(lon)) < 1e-40
    rcv = np.zeros(2, dtype=M.RECEIVER_DTYPE)
    rcv["clock_offset_s"] = [0.001, -0.001]
    c = mp.mpf(M.C_AIR)
    with mp.workdps(X.DIGITS):
        # reception times across 2^64 and ticks across 2^48: signed differences; the declared offsets come off
        r = X.rho_of(rcv, [0, 1], [(1 << 64) - 5, 7], M.TIME_RECEPTION, 1e-9)
        assert r[0] == 0 and r[1] == c * (12 * mp.mpf(1e-9) - (mp.mpf(-0.001) - mp.mpf(0.001)))
        r = X.rho_of(rcv, [1, 0], [3, (1 << 48) - 2], M.TIME_TICKS, 1 / 12e6)
        assert r[1] == c * (-5 * mp.mpf(1 / 12e6) - (mp.mpf(0.001) - mp.mpf(-0.001)))
    assert X.altitude_of(K.edge_frame(0x8D, 11, K.q_code(2047))) == mp.mpf(50175) * mp.mpf("0.3048")
    assert X.altitude_of(K.edge_frame(0x8D, 11, 0x3A8)) is None and X.altitude_of(K.edge_frame(0xA0, 11, 0x010)) is None


# ---- the bounds are the model's own; the mirror keeps its claims ----

def test_bounds_are_the_model_s(oracle):
    """The figures of the numpy model's own VALID fixes with pdop <= 20, over the case lists and the edge lists: each
    is at most the recorded one (tests/mlat_exact.py MODEL_MEASURED), whose 10-fold is the tolerance."""
    worst, n = {}, 0
    for name, rcv, lst, cfg, _, want, _, _ in K.modelled(oracle):
        n += X.check_list(name, rcv, lst, cfg, want, worst)
    print(f"the model's own fixes against the exact check, {n} fixes: " + ", ".join(
        f"{k} {worst[k]:.3g} (recorded {X.MODEL_MEASURED[k]:.3g})" for k in X.MODEL_MEASURED) +
        f", residual_rms_m above the floor {worst['residual_rms_m']:.3g}")
    assert n >= 250
    for k, v in X.MODEL_MEASURED.items():
        assert v / 1.1 <= worst[k] <= v, (k, worst[k], v)


def test_mirror_fixes_keep_their_claims(lib, oracle):
    worst, n = {}, 0
    for name, rcv, lst, cfg, _, _, _, _ in K.modelled(oracle):
        got, _ = lib.host_multilaterate(rcv, lst["msgs"], lst["recs"], lst["rx"], **cfg)
        n += X.check_list(name, rcv, lst, cfg, got, worst)
    print(f"the mirror's fixes against the exact check, {n} fixes: " + ", ".join(
        f"{k} {worst[k]:.3g} (tolerance {X.TOL[k]:.3g})" for k in X.TOL) +
        f", residual_rms_m above the floor {worst['residual_rms_m']:.3g} (tolerance "
        f"{M.MIRROR_VS_MODEL_TOL['residual_rms_m']:.3g})")
    assert n >= 250
