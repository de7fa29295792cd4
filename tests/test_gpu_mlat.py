"""Multilaterate on the device (adsb_multilaterate, adsb_multilaterate_of, adsb_fetch_mlat, adsb_mlat_device) against the
CPU mirror under the rule of tests/test_mlat_host.py (the device shares the mirror's order of operations, so the
mirror-vs-model tolerance bounds it), at the smallest shapes at which the kernel can go wrong, with lists in host and in
device memory, straight behind correlate, end to end from Beast bytes, and run to run."""
import ctypes as C

import numpy as np
import pytest

import air_rs_amd as A
from air_rs_amd import _lib
from tests import mlat_cases as K
from tests import mlat_model as M
from tests.test_mlat_host import same_fixes
from tests.traffic import ident_frame

pytestmark = pytest.mark.gpu
NS = dict(seconds_per_tick=K.SPT_NS)


def _hip_runtime():
    """The HIP runtime this process already holds (the one libadsb_hip.so is bound to), for plain device allocations."""
    for line in open("/proc/self/maps"):
        path = line.split()[-1]
        if "libamdhip64" in path:
            hip = C.CDLL(path)
            hip.hipMalloc.argtypes, hip.hipMalloc.restype = [C.POINTER(C.c_void_p), C.c_size_t], C.c_int
            hip.hipMemcpy.argtypes, hip.hipMemcpy.restype = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int], C.c_int
            hip.hipFree.argtypes, hip.hipFree.restype = [C.c_void_p], C.c_int
            return hip
    raise RuntimeError("no HIP runtime mapped")


class _Dev:
    """A host array's bytes in device memory, freed on close()."""

    def __init__(self, arr):
        arr = np.ascontiguousarray(arr)
        self._hip, self.ptr, self.n = _hip_runtime(), C.c_void_p(), len(arr)
        assert self._hip.hipMalloc(C.byref(self.ptr), max(arr.nbytes, 1)) == 0
        if arr.nbytes:
            assert self._hip.hipMemcpy(self.ptr, arr.ctypes.data, arr.nbytes, 1) == 0      # hipMemcpyHostToDevice

    def pair(self):
        return self.ptr.value, self.n

    def close(self):
        assert self._hip.hipFree(self.ptr) == 0


@pytest.fixture(scope="module")
def ctx(gpu):
    with A.AdsbDemod(max_samples=1 << 16, max_out=1024) as d:
        yield d


def _lasts(rcv, lst, cfg):
    return M.multilaterate(rcv, lst["msgs"], lst["recs"], lst["rx"], **cfg)[2]


def _check(d, rcv, lst, cfg, name, rx=False, lasts=None):
    """multilaterate_of (host lists) against the mirror; the header against the fixes.  -> (fixes, largest gap)"""
    rxa = lst["rx"] if rx or cfg.get("time_source") else None
    want, wh = A.host_multilaterate(rcv, lst["msgs"], lst["recs"], rxa, **cfg)
    got, hdr = d.multilaterate_of(rcv, lst["msgs"], lst["recs"], rxa, **cfg)
    lasts = _lasts(rcv, lst, cfg) if lasts is None else lasts
    worst = same_fixes(got, want, lasts, cfg.get("step_tol_m") or 0.01, name)
    assert int(hdr["n_messages"]) == len(got) == len(lst["msgs"]) and int(hdr["flags"]) == 0
    assert int(hdr["n_attempted"]) == int((got["flags"] & M.ATTEMPTED != 0).sum())
    assert int(hdr["n_valid"]) == int((got["flags"] & M.VALID != 0).sum())
    assert (got["reserved"] == 0).all()
    return got, worst


def test_geometry(gpu):
    lanes, per = C.c_uint32(), C.c_uint32()
    assert _lib.load().adsb_debug_mlat_geometry(C.byref(lanes), C.byref(per)) == A.ADSB_OK
    assert (lanes.value, per.value) == (16, 16)              # what the counts below are chosen for


def test_case_lists_device_vs_mirror(ctx, oracle):
    worst = 0.0
    for name, rcv, lst, cfg in K.case_lists(oracle):
        got, gap = _check(ctx, rcv, lst, cfg, name)
        worst = max(worst, gap)
        # the same lists in device memory, and run to run: the same bytes
        dm, dr, dx = _Dev(lst["msgs"]), _Dev(lst["recs"]), _Dev(lst["rx"])
        rx = dx.pair() if cfg.get("time_source") else None
        again, _ = ctx.multilaterate_of(rcv, dm.pair(), dr.pair(), rx, **cfg)
        assert again.tobytes() == got.tobytes(), name
        mixed, _ = ctx.multilaterate_of(rcv, lst["msgs"], dr.pair(), lst["rx"] if cfg.get("time_source") else None, **cfg)
        assert mixed.tobytes() == got.tobytes(), name
        for dev in (dm, dr, dx):
            dev.close()
    print(f"largest device-vs-mirror position gap over fixes with pdop <= 20: {worst:.3g} m "
          f"(tolerance {M.MIRROR_VS_MODEL_TOL_M:.3g} m)")


def test_message_counts(ctx, oracle):
    """0, 1, 3, 4, 5 (a partly filled wavefront), 15, 16, 17 (a partly filled workgroup, one, one and a bit) and 257
    (more than 16 workgroups) messages: prefixes of one list, whose fixes do not depend on the messages behind them."""
    rcv = K.receivers(6, seed=906)
    pos, frames = K.emitters(oracle, 257, seed=907)
    full = K.build(rcv, pos, frames)
    lasts = _lasts(rcv, full, NS)
    whole = None
    for n in (257, 0, 1, 3, 4, 5, 15, 16, 17):
        n_recs = int(full["msgs"]["first"][n]) if n < 257 else len(full["recs"])
        lst = {"msgs": full["msgs"][:n], "recs": full["recs"][:n_recs], "rx": full["rx"]}
        got, _ = _check(ctx, rcv, lst, NS, f"{n} messages", lasts=lasts[:n])
        whole = got if whole is None else whole
        assert got.tobytes() == whole[:n].tobytes()
    assert (whole["flags"] & M.VALID != 0).sum() >= 250


@pytest.mark.parametrize("n_rcv,alt", [(3, True), (4, False), (15, False), (16, False), (17, False), (33, True), (256, False)])
def test_receptions_per_message(ctx, oracle, n_rcv, alt):
    """Fewer receptions than lanes, exactly one per lane, one lane with two, several per lane, and the most there is."""
    rcv, lst, cfg = K.many_receivers(oracle, n_rcv, n_em=5 if n_rcv < 256 else 2)
    cfg = dict(cfg, use_altitude=alt)
    got, _ = _check(ctx, rcv, lst, cfg, f"{n_rcv} receptions")
    assert (got["n_used"] == n_rcv).all() and (got["flags"] & M.ATTEMPTED).all()


def test_too_many_and_repeats_beside_the_largest(ctx, oracle):
    rcv = K.receivers(256, seed=756)
    pos, frames = K.emitters(oracle, 3, seed=856)
    lst = K.build(rcv, pos, frames, extra=[(0, 5, 10)] + [(2, r, 3 + r) for r in range(0, 200, 2)])
    assert lst["msgs"]["n_receptions"].tolist() == [257, 256, 356]
    got, _ = _check(ctx, rcv, lst, NS, "257 / 256 / 356 receptions")
    assert got["flags"][0] == M.TOO_MANY and got["flags"][2] == M.TOO_MANY and got["n_used"][1] == 256


def test_attempted_and_not_in_one_wavefront(ctx, oracle):
    rcv = K.receivers(6, seed=916)
    pos, frames = K.emitters(oracle, 24, seed=917)
    heard = [[[0, 1], list(range(6)), [0, 1, 2], list(range(6)), [], [1, 2, 3, 4]][i % 6] for i in range(24)]
    lst = K.build(rcv, pos, frames, heard=heard, extra=[(i, 1, 50) for i in range(0, 24, 6)])
    got, _ = _check(ctx, rcv, lst, NS, "mixed wavefronts")
    assert [int(f) & (M.ATTEMPTED | M.TOO_FEW) for f in got["flags"][:6]] == \
        [M.TOO_FEW, M.ATTEMPTED, M.TOO_FEW, M.ATTEMPTED, M.TOO_FEW, M.ATTEMPTED]
    assert got["n_used"][:6].tolist() == [2, 6, 3, 6, 0, 4]
    # a receiver the list does not have, in one message of a wavefront: that message alone is refused, nothing is read
    few = rcv[:5]
    c = A.demod._mlat_cfg(**NS)
    L = _lib.load()
    assert L.adsb_multilaterate_of(ctx._h, C.byref(c), few.ctypes.data, 5, lst["msgs"].ctypes.data, 24,
                                   lst["recs"].ctypes.data, len(lst["recs"]), None, 0) == A.ADSB_OK
    fixes, n, h = np.zeros(24, dtype=M.FIX_DTYPE), C.c_size_t(), _lib.AdsbMlatHeader()
    assert L.adsb_fetch_mlat(ctx._h, fixes.ctypes.data, 24, C.byref(n), C.byref(h)) == A.ADSB_E_ARG
    want = np.zeros(24, dtype=M.FIX_DTYPE)
    assert L.adsb_host_multilaterate(C.byref(c), few.ctypes.data, 5, lst["msgs"].ctypes.data, 24, lst["recs"].ctypes.data,
                                     len(lst["recs"]), None, 0, want.ctypes.data, None) == A.ADSB_E_ARG
    assert n.value == 24 and h.flags == A.ADSB_MLAT_HDR_BAD_INDEX and h.n_messages == 24
    assert (fixes["flags"] == want["flags"]).all() and (fixes["flags"] == M.BAD_INDEX).sum() == 8
    same_fixes(fixes, want, None, 0.01, "a receiver out of range")


def test_lane_groups_with_very_different_iteration_counts(ctx, oracle):
    """Messages with an altitude (one stage) beside messages without (identification frames: two stages): the four lane groups of a wavefront leave the loop many iterations apart."""
    rcv = K.receivers(5, seed=925)
    pos, frames = K.emitters(oracle, 32, seed=926)
    frames = [ident_frame(oracle, 0x4B0000 + i, [1 + (i + k) % 26 for k in range(8)]) if i % 2 else f
              for i, f in enumerate(frames)]
    lst = K.build(rcv, pos, frames)
    cfg = dict(NS, use_altitude=True, max_iterations=60)
    got, _ = _check(ctx, rcv, lst, cfg, "iteration spread")
    assert ((got["flags"] & M.ALTITUDE != 0) == (np.arange(32) % 2 == 0)).all()
    its = got["iterations"].astype(int).reshape(-1, 4)
    assert (its.max(axis=1) - its.min(axis=1)).max() >= 5, its


def test_behind_correlate_and_isolation(ctx, oracle):
    """adsb_multilaterate straight after correlate_of is byte for byte multilaterate_of on the fetched lists, and the
    context's other results stay what they were."""
    cfg = A.synth_default(seed=77)
    iq = A.synth_fill_host(cfg, A.ADSB_SAMPLE_I8, 0, 0, 60_000)
    frames_before, _ = ctx.demod(iq)
    levels_before = ctx.levels()
    rcv = K.receivers(7, seed=936)
    pos, fr = K.emitters(oracle, 37, seed=937)
    lst = K.build(rcv, pos, fr, extra=[(3, 2, 9)])
    ctx.correlate_of_async(lst["frames"], lst["counts"], 1_000_000)
    ctx.multilaterate_async(rcv, use_altitude=True, **NS)              # nothing fetched in between
    here, hdr = ctx.fetch_mlat()
    msgs, fout, recs = ctx.fetch_correlated()
    assert msgs.tobytes() == lst["msgs"].tobytes() and recs.tobytes() == lst["recs"].tobytes()
    there, hdr2 = ctx.multilaterate_of(rcv, msgs, recs, use_altitude=True, **NS)
    assert here.tobytes() == there.tobytes() and hdr.tobytes() == hdr2.tobytes() and int(hdr["n_messages"]) == 37
    assert (here["flags"] & M.VALID != 0).sum() >= 35
    again = ctx.fetch_correlated()
    assert again[0].tobytes() == msgs.tobytes() and again[2].tobytes() == recs.tobytes() and \
        again[1].tobytes() == fout.tobytes()
    frames_after = ctx.fetch()[0]
    assert frames_after.tobytes() == frames_before.tobytes() and len(frames_before) > 10
    assert ctx.levels().tobytes() == levels_before.tobytes()
    f_dev, h_dev = ctx.mlat_device()
    assert f_dev and h_dev
    # an empty correlate result
    ctx.correlate_of_async(lst["frames"][:0], np.zeros(7, dtype=np.uint64), 10)
    none, hdr = ctx.multilaterate(rcv, **NS)
    assert len(none) == 0 and hdr.tobytes() == bytes(32)


def test_errors_on_a_context(gpu, oracle):
    rcv = K.receivers(4, seed=1)
    with A.AdsbDemod(max_samples=1 << 12, max_out=64) as d:
        with pytest.raises(A.AdsbError) as e:
            d.multilaterate_async(rcv, **NS)
        assert e.value.code == A.ADSB_E_STATE                      # before any correlate
        with pytest.raises(A.AdsbError) as e:
            d.fetch_mlat()
        assert e.value.code == A.ADSB_E_STATE
        with pytest.raises(A.AdsbError) as e:
            d.mlat_device()
        assert e.value.code == A.ADSB_E_STATE
        for bad in (dict(seconds_per_tick=0.0), dict(time_source="ticks"), dict(NS, max_iterations=1001),
                    dict(NS, step_tol_m=float("nan"))):
            with pytest.raises(A.AdsbError) as e:
                d.multilaterate_of_async(rcv, np.zeros(0, dtype=M.MESSAGE_DTYPE), np.zeros(0, dtype=M.RECEPTION_DTYPE),
                                         **bad)
            assert e.value.code == A.ADSB_E_ARG, bad
        far = rcv.copy()
        far["latitude"][1] = 91.0
        with pytest.raises(A.AdsbError) as e:
            d.multilaterate_of_async(far, np.zeros(0, dtype=M.MESSAGE_DTYPE), np.zeros(0, dtype=M.RECEPTION_DTYPE), **NS)
        assert e.value.code == A.ADSB_E_ARG


def test_end_to_end_from_beast_bytes(ctx, oracle):
    """Emitters -> each receiver's frames as Beast with its own tick bias -> wire_in_of -> correlate_of -> multilaterate
    with TIME_TICKS on the parser's rx records in device memory; the fixes against the model on the same ticks."""
    biases = np.array([0, 1201, 2402, 3607, 4804, 6005])
    rcv = K.receivers(6, seed=946, clock_offsets=biases / 12e6)
    pos, fr = K.emitters(oracle, 30, seed=947)
    plain = K.receivers(6, seed=946)                                  # the biases go in through the encoder instead
    lst = K.build(plain, pos, fr, spt=0.5e-6)                         # offsets in 2 MHz samples
    streams, ends, at = [], [], 0
    for r in range(6):
        mine = lst["frames"][at:at + int(lst["counts"][r])]
        at += len(mine)
        enc = A.host_wire_encode(mine, tick_bias=int(biases[r]))[0] if r % 2 else ctx.wire_of(mine, tick_bias=int(biases[r]))[0]
        streams.append(enc)
        ends.append(sum(len(s) for s in streams))
    win = ctx.wire_in_of(b"".join(streams), ends)
    assert win.counts.tolist() == lst["counts"].tolist()
    assert (win.rx["ticks"] == 6 * lst["frames"]["offset"] + biases[win.rx["receiver"]]).all()
    ctx.correlate_of_async(win.frames, win.counts, 5000)
    cfg = dict(time_source="ticks", use_altitude=True)
    got, hdr = ctx.multilaterate(rcv, rx=ctx.wire_in_device()[1], **cfg)
    msgs, _, recs = ctx.fetch_correlated()
    assert len(msgs) == 30 and (msgs["n_receivers"] == 6).all()
    want, _, lasts = M.multilaterate(rcv, msgs, recs, win.rx, time_source=M.TIME_TICKS, use_altitude=True)
    same_fixes(got, want, lasts, 0.01, "end to end")
    mirror, _ = A.host_multilaterate(rcv, msgs, recs, win.rx, **cfg)
    same_fixes(got, mirror, lasts, 0.01, "end to end, mirror")
    valid = got["flags"] & M.VALID != 0
    assert valid.sum() >= 25 and int(hdr["n_valid"]) == valid.sum()
    # 0.5 us ticks are 150 m of range: the fixes are near their emitters, not on them
    order = {bytes(f): i for i, f in enumerate(fr)}
    err = [float(np.sqrt(((M.ecef_of(f["latitude"], f["longitude"], f["height_m"]) - pos[order[bytes(m["bytes"])]]) ** 2).sum()))
           for f, m in zip(got[valid], msgs[valid])]
    assert max(err) < 150.0 * 3 * float(got["pdop"][valid].max()) and np.median(err) < 5000.0
