"""Multilaterate ON THE DEVICE at the outcomes and cfg fields its other suite never reaches (tests/mlat_cases.edge_lists:
SINGULAR, both rejections, min_receivers, iteration caps and step tolerances, default_altitude_m, declared offsets, the
2^48 / 2^63 / 2^64 time wraps, the altitude decode's edges, poles, antimeridian and equator), on the known-truth lists,
and with all of them side by side in one wavefront.  Every list goes through same_fixes against the CPU mirror (every
output field, no message left out), the header checks of tests/test_gpu_mlat.py, the list's literal expectations and a
second run for the same bytes; every VALID fix with pdop <= 20 then has to keep what it claims under the exact check of
tests/mlat_exact.py, which knows the inputs and not the solver."""
import numpy as np
import pytest

import air_rs_amd as A
from tests import mlat_cases as K
from tests import mlat_exact as X
from tests import mlat_model as M
from tests.test_gpu_mlat import _check
from tests.test_mlat_host import same_fixes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(gpu):
    with A.AdsbDemod(max_samples=1 << 16, max_out=1024) as d:
        yield d


def _rx(lst, cfg):
    return lst["rx"] if cfg.get("time_source") else None


@pytest.fixture(scope="module")
def device(ctx, oracle):
    """{name: (fixes, header)} of every case list and edge list on the device, each run once."""
    return {name: ctx.multilaterate_of(rcv, lst["msgs"], lst["recs"], _rx(lst, cfg), **cfg)
            for name, rcv, lst, cfg, *_ in K.modelled(oracle)}


def _say(what, gaps):
    print(f"largest {what} gaps over fixes with pdop <= 20: " + ", ".join(
        f"{k} {gaps.get(k, 0.0):.3g} (tolerance {tol:.3g})" for k, tol in M.MIRROR_VS_MODEL_TOL.items()))


def test_edge_lists_device_vs_mirror(ctx, oracle, device):
    worst, gaps, results = 0.0, {}, {}
    for name, rcv, lst, cfg, expect, want, want_hdr, lasts in K.modelled(oracle):
        if expect is None:
            continue
        got, gap = _check(ctx, rcv, lst, cfg, name, lasts=lasts)
        worst = max(worst, gap)
        mirror, _ = A.host_multilaterate(rcv, lst["msgs"], lst["recs"], _rx(lst, cfg), **cfg)
        tol = cfg.get("step_tol_m") or 0.01
        same_fixes(got, mirror, lasts, tol, name, gaps=gaps)
        # no message is left out of the comparison: every integer is the mirror's
        assert got["flags"].tolist() == mirror["flags"].tolist() and got["n_used"].tolist() == mirror["n_used"].tolist() \
            and got["iterations"].tolist() == mirror["iterations"].tolist(), name
        assert got.tobytes() == device[name][0].tobytes(), name                       # run to run
        results[name] = got
        error = K.check_expectations(name, want, want_hdr, expect, {}, lasts, tol) if "truth" in expect else None
        mine = K.check_expectations(name, got, device[name][1], expect, results, lasts, tol, model_error=error)
        if error is not None:
            print(f"{name}: largest error against the truth, model {error:.2f} m, device {mine:.2f} m")
    print(f"largest device-vs-mirror position gap over the edge lists: {worst:.3g} m "
          f"(tolerance {M.MIRROR_VS_MODEL_TOL_M:.3g} m)")
    _say("device-vs-mirror (edge lists)", gaps)


def test_case_lists_every_field(ctx, oracle, device):
    """The case lists of tests/test_gpu_mlat.py again, for the print of the gap per field."""
    gaps = {}
    for name, rcv, lst, cfg, expect, _, _, lasts in K.modelled(oracle):
        if expect is None:
            mirror, _ = A.host_multilaterate(rcv, lst["msgs"], lst["recs"], _rx(lst, cfg), **cfg)
            same_fixes(device[name][0], mirror, lasts, 0.01, name, gaps=gaps)
    _say("device-vs-mirror (case lists)", gaps)


def test_one_wavefront_one_message_at_a_time(ctx, oracle, device):
    """A fix does not depend on its neighbours in the wavefront: the 16 messages of four kinds, run as 16 lists of one
    message, give the same bytes."""
    name, rcv, lst, cfg, expect = K.one_wavefront(oracle)
    whole = device[name][0]
    assert expect["one_at_a_time"] and len(whole) == 16
    for g in range(16):
        alone, hdr = ctx.multilaterate_of(rcv, lst["msgs"][g:g + 1], lst["recs"], **cfg)
        assert len(alone) == 1 and alone.tobytes() == whole[g:g + 1].tobytes(), g
        assert int(hdr["n_valid"]) == int(whole["flags"][g] & M.VALID != 0)
    mirror, _ = A.host_multilaterate(rcv, lst["msgs"], lst["recs"], **cfg)
    for g in range(16):                                                  # per message against the mirror
        same_fixes(whole[g:g + 1], mirror[g:g + 1], None, 0.01, f"{name}, message {g}")


@pytest.fixture(scope="module")
def truth_lasts(oracle):
    out = {}
    for row in K.TRUTH_ROWS:
        rcv, lst, cfg, pos, err = K.truth_list(oracle, row[0])
        part = {"msgs": lst["msgs"][:100], "recs": lst["recs"][:int(lst["msgs"]["first"][100])], "rx": lst["rx"]}
        out[row[0]] = (rcv, part, cfg, pos[:100], err, M.multilaterate(rcv, part["msgs"], part["recs"], **cfg)[2])
    return out


@pytest.mark.parametrize("row", K.TRUTH_ROWS, ids=[r[0] for r in K.TRUTH_ROWS])
def test_truth_on_the_device(ctx, truth_lasts, row):
    """The first 100 emitters of each truth list: at least 99 VALID, every valid fix within the row's 3 x err of its true
    position (the bound of tests/test_mlat_host.py::test_truth), and the mirror's fixes."""
    rcv, lst, cfg, pos, err, lasts = truth_lasts[row[0]]
    got, _ = _check(ctx, rcv, lst, cfg, row[0], lasts=lasts)
    valid = got["flags"] & M.VALID != 0
    assert len(got) == 100 and valid.sum() >= 99
    assert ((got["flags"] & M.ALTITUDE != 0) == cfg["use_altitude"]).all()
    gaps = [float(np.sqrt(((M.ecef_of(f["latitude"], f["longitude"], f["height_m"]) - p) ** 2).sum()))
            for f, p in zip(got[valid], pos[valid])]
    print(f"{row[0]}: {valid.sum()} of 100 valid, largest 3-D error {max(gaps):.2f} m, bound {3 * err:.1f} m")
    assert max(gaps) <= 3 * err


def test_device_fixes_keep_their_claims(oracle, device):
    """tests/mlat_exact.py over every VALID fix with pdop <= 20 of the case lists and the edge lists."""
    worst, n = {}, 0
    for name, rcv, lst, cfg, *_ in K.modelled(oracle):
        n += X.check_list(name, rcv, lst, cfg, device[name][0], worst)
    print(f"the device's fixes against the exact check, {n} fixes: " + ", ".join(
        f"{k} {worst[k]:.3g} (tolerance {X.TOL[k]:.3g})" for k in X.TOL) +
        f", residual_rms_m above the floor {worst['residual_rms_m']:.3g} (tolerance "
        f"{M.MIRROR_VS_MODEL_TOL['residual_rms_m']:.3g})")
    assert n >= 250
