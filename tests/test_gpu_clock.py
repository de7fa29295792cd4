"""Clock sync on the device (adsb_clock_sync, adsb_clock_sync_of, adsb_fetch_clocks, adsb_clock_apply and the device
views) against the CPU mirror, the numpy model and the truth, under the rules of tests/test_clock_host.py, at the
smallest shapes at which each kernel can go wrong, with lists in host and in device memory, straight behind correlate, and
run to run."""
import ctypes as C

import numpy as np
import pytest

import air_rs_amd as A
from air_rs_amd import _lib
from tests import clock_cases as CC
from tests import clock_model as CM
from tests import mlat_model as M
from tests import test_clock_host as H
from tests.test_gpu_mlat import _Dev

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(gpu):
    with A.AdsbDemod(max_samples=1 << 16, max_out=4096) as d:
        yield d


@pytest.fixture(scope="module")
def cases(oracle):
    return CC.case_lists(oracle)


def device_sync(d):
    return lambda rcv, lst, **cfg: d.clock_sync_of(rcv, lst["msgs"], lst["recs"], lst["rx"], **cfg)


def test_geometry(gpu):
    per, parts = C.c_uint32(), C.c_uint32()
    assert _lib.load().adsb_debug_clock_geometry(C.byref(per), C.byref(parts)) == A.ADSB_OK
    assert (per.value, parts.value) == (16, 64)              # what the counts of test_clock_host.shape_lists are chosen for


def test_case_lists_device_vs_mirror_and_model(ctx, cases):
    worst, left_out = [0.0, 0.0], 0
    for name, sc, kw in cases:
        lst, cfg = sc["lst"], dict(sc["cfg"], **kw)
        got, gh = ctx.clock_sync_of(sc["rcv"], lst["msgs"], lst["recs"], lst["rx"], **cfg)
        corrected = ctx.clock_apply()
        want, wh = H.mirror_sync(sc["rcv"], lst, **cfg)
        da, db = H.same_clocks(got, gh, want, wh, sc["rcv"]["clock_offset_s"], CM.DEVICE_VS_MIRROR_TOL_S, CM.DEVICE_VS_MIRROR_TOL_DRIFT, name)
        print(f"{name}: device vs mirror {da:.3g} s, {db:.3g} s/s")
        worst = [max(worst[0], da), max(worst[1], db)]
        model, mh = H.model_sync(sc["rcv"], lst, **cfg)[:2]
        H.same_clocks(got, gh, model, mh, sc["rcv"]["clock_offset_s"], CM.MIRROR_VS_MODEL_TOL_S + CM.DEVICE_VS_MIRROR_TOL_S,
                      CM.MIRROR_VS_MODEL_TOL_DRIFT + CM.DEVICE_VS_MIRROR_TOL_DRIFT, name)
        left_out += H.check_apply(corrected, sc, got, name)
        # the same lists in device memory, and run to run: the same bytes
        dm, dr, dx = _Dev(lst["msgs"]), _Dev(lst["recs"]), _Dev(lst["rx"])
        again, ah = ctx.clock_sync_of(sc["rcv"], dm.pair(), dr.pair(), dx.pair(), **cfg)
        assert again.tobytes() == got.tobytes() and ah.tobytes() == gh.tobytes(), name
        assert ctx.clock_apply().tobytes() == corrected.tobytes(), name
        mixed, _ = ctx.clock_sync_of(sc["rcv"], lst["msgs"], dr.pair(), lst["rx"], **cfg)
        assert mixed.tobytes() == got.tobytes(), name
        for dev in (dm, dr, dx):
            dev.close()
    print(f"largest device-vs-mirror gap: offset {worst[0]:.3g} s (measured {CM.DEVICE_VS_MIRROR_MEASURED_S:.3g}, "
          f"tolerance {CM.DEVICE_VS_MIRROR_TOL_S:.3g}), drift {worst[1]:.3g} (measured "
          f"{CM.DEVICE_VS_MIRROR_MEASURED_DRIFT:.3g}, tolerance {CM.DEVICE_VS_MIRROR_TOL_DRIFT:.3g}); receptions left "
          f"out of the corrected-time comparison: {left_out}")


def test_polar_antimeridian_scenario(ctx, oracle):
    H.check_polar(device_sync(ctx), oracle, H.mirror_sync, CM.DEVICE_VS_MIRROR_TOL_S, CM.DEVICE_VS_MIRROR_TOL_DRIFT,
                  "device vs mirror")
    H.check_polar(device_sync(ctx), oracle, H.model_sync, CM.MIRROR_VS_MODEL_TOL_S + CM.DEVICE_VS_MIRROR_TOL_S,
                  CM.MIRROR_VS_MODEL_TOL_DRIFT + CM.DEVICE_VS_MIRROR_TOL_DRIFT, "device vs model")


def test_shapes(ctx, oracle):
    for name, sc, kw, expect in H.shape_lists(oracle):
        H.check_shape(device_sync(ctx), name, sc, kw, expect, CM.DEVICE_VS_MIRROR_TOL_S, CM.DEVICE_VS_MIRROR_TOL_DRIFT,
                      reference_sync=H.mirror_sync)
        lst = sc["lst"]
        corrected = ctx.clock_apply()
        clocks = ctx.fetch_clocks()[0]
        mirror = A.host_clock_apply(clocks, lst["msgs"], lst["recs"], lst["rx"], **sc["cfg"])
        assert corrected.tobytes() == mirror.tobytes(), name     # the same clocks in: the same integers out


@pytest.mark.parametrize("name", [r[0] for r in H.TRUTH_ROWS])
def test_truth(ctx, oracle, name):
    H.check_truth(device_sync(ctx), oracle, name)


def test_outliers(ctx, oracle):
    """The device's dropped SET is the model's: the device's own first-pass clocks put the same slots beyond the limit
    (the residual rule applied in Python to the model's rows, whose y agree with the device's to the last bits and lie
    at least 1e-9 s from the limit), and its second pass drops exactly that many rows per receiver and in all."""
    H.check_outliers(device_sync(ctx), oracle)
    sc, planted = CC.outliers(oracle)
    lst = sc["lst"]
    cfg = dict(sc["cfg"], max_residual_s=H.OUTLIER_LIMIT_S)
    _, _, state, _ = H.model_sync(sc["rcv"], lst, **cfg)
    first = ctx.clock_sync_of(sc["rcv"], lst["msgs"], lst["recs"], lst["rx"], **sc["cfg"])[0]
    rows = CM.rows_of(sc["rcv"], lst["msgs"], lst["recs"], lst["rx"], **sc["cfg"])[0]
    beyond = {r["slot"] for r in rows if abs(CM.residual(r, first["fine_offset_s"], first["drift"])) > H.OUTLIER_LIMIT_S}
    assert beyond == set(np.flatnonzero(state == 2).tolist()) and len(beyond) > 0
    got, gh = ctx.clock_sync_of(sc["rcv"], lst["msgs"], lst["recs"], lst["rx"], **cfg)
    assert int(gh["n_dropped"]) == len(beyond)
    per = np.zeros(len(sc["rcv"]), dtype=np.int64)
    for r in rows:
        if r["slot"] in beyond:
            per[r["i"]] += 1
            per[r["j"]] += 1
    assert (got["n_dropped"] == per).all()


def test_bad_index(ctx, oracle):
    """The header flag is set, nothing is read (the run ends clean) and the other messages are still used."""
    L = _lib.load()
    for name, sc, lst in H.bad_index_lists(oracle):
        want, wh = H.model_sync(sc["rcv"], lst, **sc["cfg"])[:2]
        c = A.demod._clock_cfg(**sc["cfg"])
        assert L.adsb_clock_sync_of(ctx._h, C.byref(c), sc["rcv"].ctypes.data, 4, lst["msgs"].ctypes.data, len(lst["msgs"]),
                                    lst["recs"].ctypes.data, len(lst["recs"]), lst["rx"].ctypes.data,
                                    len(lst["rx"])) == A.ADSB_OK, name
        clocks, hdr, n = np.zeros(4, dtype=A.CLOCK_DTYPE), _lib.AdsbClockHeader(), C.c_size_t()
        assert L.adsb_fetch_clocks(ctx._h, clocks.ctypes.data, 4, C.byref(n), C.byref(hdr)) == A.ADSB_E_ARG, name
        assert n.value == 4 and hdr.flags == CM.HDR_BAD_INDEX and hdr.n_eligible == 19 and hdr.n_rows == 57, name
        mirror = np.zeros(4, dtype=A.CLOCK_DTYPE)
        assert L.adsb_host_clock_sync(C.byref(c), sc["rcv"].ctypes.data, 4, lst["msgs"].ctypes.data, len(lst["msgs"]),
                                      lst["recs"].ctypes.data, len(lst["recs"]), lst["rx"].ctypes.data, len(lst["rx"]),
                                      mirror.ctypes.data, None, None) == A.ADSB_E_ARG
        assert np.abs(clocks["fine_offset_s"] - mirror["fine_offset_s"]).max() <= CM.DEVICE_VS_MIRROR_TOL_S, name
        assert (clocks["n_rows"] == mirror["n_rows"]).all() and (clocks["flags"] == mirror["flags"]).all(), name
        corrected = ctx.clock_apply()
        want_c = A.host_clock_apply(clocks, lst["msgs"], lst["recs"], lst["rx"], **sc["cfg"])
        assert corrected.tobytes() == want_c.tobytes(), name


def test_behind_correlate_same_ctx_and_isolation(ctx, oracle):
    """The context's other results -- frames, levels, wire input, correlate, multilaterate -- are fetched BEFORE any clock
    call and are the same bytes after adsb_clock_sync, adsb_clock_sync_of and adsb_clock_apply, with no correlate or
    multilaterate call in between.  adsb_clock_sync straight behind correlate is byte for byte clock_sync_of on the
    fetched lists; two runs on one ctx give the same bytes; multilaterate(clocks=True) is the solver on the corrected
    list."""
    cfg = A.synth_default(seed=78)
    iq = A.synth_fill_host(cfg, A.ADSB_SAMPLE_I8, 0, 0, 60_000)
    frames_before, _ = ctx.demod(iq)
    levels_before = ctx.levels()
    sc = H.end_to_end_list(oracle)
    lst = sc["lst"]
    beast = A.host_wire_encode(lst["frames"][:50])[0]
    win_before = ctx.wire_in_of(beast, [len(beast)])
    ctx.correlate_of_async(lst["frames"], lst["counts"], 200_000)
    mlat_before, mlat_hdr_before = ctx.multilaterate(sc["rcv"], rx=lst["rx"], time_source="ticks", use_altitude=True)
    msgs, fout, recs = ctx.fetch_correlated()
    assert len(msgs) == len(lst["msgs"]) and int(msgs["n_receptions"].sum()) == len(lst["recs"]) == len(recs)
    assert int(mlat_hdr_before["n_attempted"]) > 100

    def others_unchanged(after):
        m, f, r = ctx.fetch_correlated()
        assert m.tobytes() == msgs.tobytes() and f.tobytes() == fout.tobytes() and r.tobytes() == recs.tobytes(), after
        fixes, hdr = ctx.fetch_mlat()
        assert fixes.tobytes() == mlat_before.tobytes() and hdr.tobytes() == mlat_hdr_before.tobytes(), after
        assert ctx.fetch()[0].tobytes() == frames_before.tobytes() and len(frames_before) > 10, after
        assert ctx.levels().tobytes() == levels_before.tobytes(), after
        win = ctx.fetch_wire_in()
        assert win.frames.tobytes() == win_before.frames.tobytes() and win.rx.tobytes() == win_before.rx.tobytes(), after

    ctx.clock_sync_async(sc["rcv"], lst["rx"], **sc["cfg"])             # on the ctx's correlate result, where it lies
    ctx.clock_apply_async()
    here, hh = ctx.fetch_clocks()
    corrected_here = ctx.clock_apply()
    assert int(hh["n_reached"]) == 9 and int(hh["n_rows"]) > 300
    others_unchanged("clock_sync and clock_apply")
    two_pass = dict(sc["cfg"], max_residual_s=1e-7)                      # both passes; drops 5 of 734 rows
    there, th = ctx.clock_sync_of(sc["rcv"], msgs, recs, lst["rx"], **two_pass)
    assert int(th["n_dropped"]) > 0
    ctx.clock_apply()
    others_unchanged("clock_sync_of with two passes and clock_apply")
    there, th = ctx.clock_sync_of(sc["rcv"], msgs, recs, lst["rx"], **sc["cfg"])
    assert here.tobytes() == there.tobytes() and hh.tobytes() == th.tobytes()
    corrected = ctx.clock_apply()
    assert corrected.tobytes() == corrected_here.tobytes()
    twice, _ = ctx.clock_sync_of(sc["rcv"], msgs, recs, lst["rx"], **sc["cfg"])
    assert twice.tobytes() == there.tobytes()
    ctx.clock_apply_async()                                              # a new sync ends the earlier apply's state
    k_dev, h_dev = ctx.clocks_device()
    assert k_dev and h_dev and ctx.clock_receptions_device()[0]
    others_unchanged("clock_sync_of, twice")
    # the solver on the corrected receptions, by hand and through multilaterate(clocks=True): these replace the
    # multilaterate result, so they come after the checks above
    plain = sc["rcv"].copy()
    plain["clock_offset_s"] = 0.0
    by_hand, _ = ctx.multilaterate_of(plain, msgs, corrected, None, seconds_per_tick=sc["spt"] / 256, use_altitude=True)
    in_one, _ = ctx.multilaterate(sc["rcv"], rx=lst["rx"], clocks=True, clock_cfg=dict(seconds_per_time=sc["spt"]),
                                  time_source="ticks", use_altitude=True)
    assert in_one.tobytes() == by_hand.tobytes() and in_one.tobytes() != mlat_before.tobytes()
    # an empty correlate result
    ctx.correlate_of_async(lst["frames"][:0], np.zeros(9, dtype=np.uint64), 10)
    none, hdr = ctx.clock_sync(sc["rcv"], seconds_per_tick=1e-6)
    assert len(none) == 9 and int(hdr["n_messages"]) == 0 and int(hdr["n_reached"]) == 1 and len(ctx.clock_apply()) == 0


def test_end_to_end(ctx, oracle):
    sc = H.end_to_end_list(oracle)
    lst = sc["lst"]
    clocks, _ = ctx.clock_sync_of(sc["rcv"], lst["msgs"], lst["recs"], lst["rx"], **sc["cfg"])
    corrected = ctx.clock_apply()
    ta, _ = CC.truth(sc)
    model = H.model_sync(sc["rcv"], lst, **sc["cfg"])[0]
    H.check_end_to_end(sc, clocks, corrected, ctx.multilaterate_of, 2 * np.abs(model["fine_offset_s"] - ta).max())


def test_errors_on_a_context(gpu, oracle):
    sc = CC.scenario(oracle, 4, 4, seed=99, p_heard=1.0)
    lst = sc["lst"]
    with A.AdsbDemod(max_samples=1 << 12, max_out=64) as d:
        for call in (d.clock_apply_async, d.fetch_clocks, d.clocks_device, d.clock_receptions_device,
                     lambda: d.clock_sync_async(sc["rcv"], lst["rx"], **sc["cfg"])):     # the last: before any correlate
            with pytest.raises(A.AdsbError) as e:
                call()
            assert e.value.code == A.ADSB_E_STATE
        d.clock_sync_of(sc["rcv"], lst["msgs"], lst["recs"], lst["rx"], **sc["cfg"])
        with pytest.raises(A.AdsbError) as e:
            d.clock_receptions_device()                              # a sync, but no apply yet
        assert e.value.code == A.ADSB_E_STATE
        for bad in (dict(reference=4), dict(seconds_per_time=0.0), dict(max_residual_s=-1.0), dict(max_range_nm=float("nan")),
                    dict(seconds_per_tick=float("inf")), dict(time_source=2)):
            with pytest.raises(A.AdsbError) as e:
                d.clock_sync_of_async(sc["rcv"], lst["msgs"], lst["recs"], lst["rx"], **dict(sc["cfg"], **bad))
            assert e.value.code == A.ADSB_E_ARG, bad
        c = A.demod._clock_cfg(**sc["cfg"])
        c.flags = 2                                                   # an unknown flag
        assert _lib.load().adsb_clock_sync_of(d._h, C.byref(c), sc["rcv"].ctypes.data, 4, None, 0, None, 0,
                                              lst["rx"].ctypes.data, len(lst["rx"])) == A.ADSB_E_ARG
