"""Correlate on the device (adsb_correlate_launch, adsb_correlate_of, adsb_fetch_correlated, adsb_correlated_device):
messages, frames and receptions are compared byte for byte with the independent model (tests/correlate_model.py) at
every list size at which the kernels take another path, on the edge lists of the CPU tier, with one group longer than
two workgroups, with lists in host and in device memory, through a launch, and through the consumers the frame list is
for (one TrackTable, wire_of)."""
import ctypes as C
import math

import numpy as np
import pytest

import air_rs_amd as A
from air_rs_amd import _lib
from tests import correlate_cases as K
from tests import correlate_model as M
from tests import finish_cases as FC
from tests import wire_model as W
from tests.traffic import ident_frame, position_frame

pytestmark = pytest.mark.gpu


def _geometry():
    b = C.c_uint32()
    assert _lib.load().adsb_debug_correlate_geometry(C.byref(b)) == A.ADSB_OK
    return b.value


def _dev(arr):
    import torch
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).reshape(-1)).cuda()


def _hip_runtime():
    """The HIP runtime this process already holds (the one libadsb_hip.so is bound to), for a plain hipMemcpy."""
    for line in open("/proc/self/maps"):
        path = line.split()[-1]
        if "libamdhip64" in path:
            return C.CDLL(path)
    raise RuntimeError("no HIP runtime mapped")


def _read_device(ptr, dtype, n):
    out = np.zeros(max(n, 1), dtype=dtype)
    hip = _hip_runtime()
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipMemcpy.restype = C.c_int
    if n:
        assert hip.hipMemcpy(out.ctypes.data, ptr, dtype.itemsize * n, 2) == 0           # hipMemcpyDeviceToHost
    return out[:n]


def _device_result(d):
    """(messages, frames, receptions) read where correlated_device() says they are, after the stream has drained."""
    msgs, _, recs = d.fetch_correlated()                                                  # waits
    m, f, r, h = d.correlated_device()
    hdr = _read_device(h, np.dtype("<u8"), 2)
    assert hdr.tolist() == [len(msgs), len(recs)]
    return (_read_device(m, M.MESSAGE_DTYPE, len(msgs)), _read_device(f, M.FRAME_DTYPE, len(msgs)),
            _read_device(r, M.RECEPTION_DTYPE, len(recs)))


def _check(d, fr, counts, w, base, lv, what, want=None):
    """correlate_of against the model: the fetched arrays and the device arrays (frames_out among them)."""
    want = M.correlate(fr, counts, w, base, lv) if want is None else want
    M.same(d.correlate_of(fr, counts, w, base, lv), want, what)
    M.same(_device_result(d), want, (what, "device arrays"))
    return want


@pytest.fixture(scope="module")
def ctx(gpu):
    with A.AdsbDemod(max_samples=1 << 16, max_out=1024) as d:
        yield d


# ---- 1: every size at which a kernel takes another path ----------------------------------------------------------------
def test_sizes(ctx):
    b = _geometry()
    for n in (0, 1, b - 1, b, b + 1, 2 * b + 3):
        fr, counts, lv = M.random_list(n, 5, seed=100 + n)
        base = [11 * r for r in range(5)]
        with_lv = _check(ctx, fr, counts, 40, base, lv, (n, "host, levels"))
        no_lv = _check(ctx, fr, counts, 40, base, None, (n, "host, no levels"))
        if n >= b:
            sizes = set(with_lv[0]["n_receptions"].tolist())
            assert {1, 2, 3} <= sizes and max(sizes) >= 4 and with_lv[0]["n_receivers"].max() >= 4, sizes
        dfr, dlv = _dev(fr), _dev(lv)
        M.same(ctx.correlate_of((dfr.data_ptr(), n), counts, 40, base, dlv.data_ptr()), with_lv, (n, "device, device"))
        M.same(ctx.correlate_of((dfr.data_ptr(), n), counts, 40, base, lv), with_lv, (n, "device, host"))
        M.same(ctx.correlate_of(fr, counts, 40, base, dlv.data_ptr()), with_lv, (n, "host, device"))
        M.same(ctx.correlate_of((dfr.data_ptr(), n), counts, 40, base), no_lv, (n, "device, none"))
        # run to run: the same bytes
        one, two = ctx.correlate_of(fr, counts, 40, base, lv), ctx.correlate_of(fr, counts, 40, base, lv)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(one, two))
        M.same(ctx.correlate_of(fr, counts, 40, base, lv), A.host_correlate(fr, counts, 40, base, lv), (n, "mirror"))
        del dfr, dlv


# ---- 2, 4, 5, 6, 7: the edge lists of the CPU tier -----------------------------------------------------------------------
CASES = K.chain_cases() + K.key_cases() + K.time_cases() + K.receiver_cases() + K.status_level_cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_edge_lists(ctx, case):
    name, fr, counts, w, base, lv = case
    _check(ctx, fr, counts, w, base, lv, name)


# ---- 3: one group longer than two workgroups ----------------------------------------------------------------------------
def _long_group(n, split_at=None, window=3):
    """n receptions of the same bytes over 3 receivers, one sample apart (a chain); split_at: the reception at that
    position of group order comes window + 1 samples late and everything behind it 2 x (window + 1), so the gaps on
    both sides of it are window + 2 -- it is a group of its own between two long ones."""
    per = [[] for _ in range(3)]
    for k in range(n):
        t = 1000 + k
        if split_at is not None and k >= split_at:
            t += window + 1 + (window + 1 if k > split_at else 0)
        status = 1 if k % 5 == 0 else 0
        per[k % 3].append((t, K.KNOWN, status, k % 88 if status else 0xFF, (k * 7919) % 1000, int(k % 4 != 0)))
    return M.build(per, levels=True)


def test_one_group_longer_than_two_workgroups(ctx):
    """`Planted at position p of group order`: a frame with other bytes sorts to an end of group order, never into the
    middle of a run of equal bytes, so the plant that lands at p is one with the same bytes and a gap above the window
    on both sides; a frame with other bytes is planted at LIST index p as well (the long group then has a member less
    in the middle, and the list indices of its receptions skip p)."""
    b = _geometry()
    n, w = 2 * b + 5, 3
    fr, counts, lv = _long_group(n)
    want = _check(ctx, fr, counts, w, None, lv, "one group")
    m = want[0]
    ks = np.arange(n)
    assert len(m) == 1 and m["n_receptions"][0] == n and m["n_receivers"][0] == 3 and m["span"][0] == n - 1
    assert m["n_clean"][0] == int((ks % 5 != 0).sum()) and m["status"][0] == 0 and m["first"][0] == 0
    sums = np.where(ks % 4 != 0, (ks * 7919) % 1000, -1)
    assert m["best_signal_sum"][0] == sums.max() and m["best_receiver"][0] == int(sums.argmax()) % 3
    assert want[2]["frame"].tolist() != list(range(n)) and sorted(want[2]["frame"].tolist()) == list(range(n))
    _check(ctx, fr, counts, w, None, None, "one group, no levels")
    for p in (b - 1, b, b + 1):
        fr, counts, lv = _long_group(n, split_at=p)
        want = _check(ctx, fr, counts, w, None, lv, ("split", p))
        assert want[0]["n_receptions"].tolist() == [p, 1, n - p - 1] and want[0]["first"].tolist() == [0, p, p + 1]
        # other bytes at list index p: smaller than KNOWN (first in group order), then greater (last)
        for other in (bytes(14), bytes([0xFF] * 14)):
            fr, counts, lv = _long_group(n)
            fr["bytes"][p] = np.frombuffer(other, dtype=np.uint8)
            want = _check(ctx, fr, counts, w, None, lv, ("other bytes", p, other[0]))
            assert sorted(want[0]["n_receptions"].tolist()) == [1, n - 1]     # the gap it leaves (2) is inside the window


# ---- 8: from a launch ---------------------------------------------------------------------------------------------------
def _shifted_channels(n, delays, constant=None):
    """The same synthetic stream on every channel, channel k starting delays[k] samples later."""
    cfg = A.synth_default(seed=3, slot_len=800)
    whole = A.synth_fill_host(cfg, A.ADSB_SAMPLE_I8, 0, 0, n + max(delays)).copy()
    for k, dk in enumerate(delays):
        assert (whole[dk:dk + 4096] == A.synth_fill_host(cfg, A.ADSB_SAMPLE_I8, 0, dk, 4096)).all()
    if constant is not None:
        whole[constant[0]:constant[1]] = (3, 4)       # one frame per offset: tiles far over their slots
    return np.concatenate([whole[dk:dk + n] for dk in delays])


@pytest.mark.parametrize("rebuild", [False, True], ids=["plain", "pool_limit"])
def test_from_a_launch(gpu, rebuild):
    n, delays = 50_000, [0, 1234, 4321]
    buf = _shifted_channels(n, delays, (30_000, 31_500) if rebuild else None)
    dev = _dev(buf)
    with A.AdsbDemod(max_samples=n, max_out=1 << 14, max_channels=3, host_staging=False) as d:
        L = _lib.load()
        cfg = _lib.AdsbCorrelateCfg(0, 0, 0)
        assert L.adsb_correlate_launch(d.handle, C.byref(cfg), None) == A.ADSB_E_STATE          # before any launch
        assert L.adsb_fetch_correlated(d.handle, None, 0, None, None, 0, None) == A.ADSB_E_STATE
        assert L.adsb_correlated_device(d.handle, None, None, None, None) == A.ADSB_E_STATE
        d.pool_limit(rebuild)
        d.demod_device_async(dev.data_ptr(), n, n_channels=3, channel_stride=n)
        got = d.correlate(0, delays)                            # the wait in it rebuilds a list with holes
        d.pool_limit(False)
        frames, counts, total, flags = d.fetch()
        assert flags == 0 and len(frames) == total and min(counts) > (1000 if rebuild else 30)
        want = M.correlate(frames, counts, 0, delays)
        M.same(got, want, "window 0")
        M.same(_device_result(d), want, "window 0, device arrays")
        msgs = want[0]
        inside = (msgs["time"] >= max(delays)) & (msgs["time"] + 240 <= n + min(delays))
        assert inside.sum() > (1000 if rebuild else 30)
        assert (msgs["n_receivers"][inside] == 3).all() and (msgs["span"][inside] == 0).all()
        assert (msgs["n_receptions"][inside] == 3).all() and len(msgs) < len(frames) / 2
        # with the launch's levels (enqueued by the call)
        got = d.correlate(0, delays, levels=True)
        lv = d.levels()
        want = M.correlate(frames, counts, 0, delays, lv)
        M.same(got, want, "levels")
        recs = want[2]
        for m in want[0][:200]:
            mine = recs["frame"][int(m["first"]):int(m["first"]) + int(m["n_receptions"])]
            valid = [int(lv["signal_sum"][j]) for j in mine if lv["flags"][j] & A.ADSB_LEVEL_VALID]
            assert m["best_signal_sum"] == (max(valid) if valid else 0)
        assert (want[0]["best_receiver"] != 0xFFFF).sum() > 30
        # a wider window joins no more here than equal times do, and never fewer receptions
        M.same(d.correlate(100, delays), M.correlate(frames, counts, 100, delays), "window 100")
    del dev


# ---- 8b: a launch of as many channels as correlate takes receivers, and of one more ---------------------------------------
def test_from_a_launch_of_256_and_257_channels(gpu, oracle):
    """One-tile channels from the pool of tests/finish_cases.py, channel k as receiver k.  256 channels: what
    correlate_of makes of the fetched list and counts (and the model).  257: ADSB_E_ARG, and the result of the call
    before stays."""
    L = _lib.load()
    n = FC.SAMPLES
    p = FC.pool(oracle, A.ADSB_SAMPLE_I8, n)
    perm = np.random.default_rng(257).integers(0, len(p.counts), 257)
    perm[255:] = np.nonzero(p.counts >= 2)[0][:2]                    # the last receiver of either launch has frames
    c = FC.case_of(p, perm)
    dev = _dev(np.ascontiguousarray(p.iq[c.perm]))
    with A.AdsbDemod(max_samples=n, max_out=int(c.prefix[-1]) + 16, max_channels=257, host_staging=False) as d:
        d.demod_device_async(dev.data_ptr(), n, n_channels=256, channel_stride=n)
        base = [k % 3 for k in range(256)]                           # within the window: equal entries join across channels
        got = d.correlate(2, base)
        frames, counts, total, flags = d.fetch()
        assert flags == 0 and total == len(frames) == c.prefix[256] and frames.tobytes() == c.frames[:total].tobytes()
        assert list(counts) == c.counts[:256].tolist() and counts[255] > 0
        want = M.correlate(frames, counts, 2, base)
        M.same(got, want, "256 channels")
        M.same(d.correlate_of(frames, counts, 2, base), want, "correlate_of")
        assert want[0]["n_receivers"].max() > 1 and len(want[0]) < len(frames)
        kept = d.fetch_correlated()
        d.demod_device_async(dev.data_ptr(), n, n_channels=257, channel_stride=n)
        cfg = _lib.AdsbCorrelateCfg(2, 0, 0)
        assert L.adsb_correlate_launch(d.handle, C.byref(cfg), None) == A.ADSB_E_ARG
        M.same(d.fetch_correlated(), kept, "the rejected launch leaves the result")
        M.same(_device_result(d), want, "and the device arrays")
        frames, counts, total, flags = d.fetch()                     # the launch itself is whole
        assert flags == 0 and frames.tobytes() == c.frames.tobytes() and list(counts) == c.counts.tolist()
    del dev


# ---- 9: what it is for --------------------------------------------------------------------------------------------------
def _cpr(oracle, lat, lon, odd):
    dlat = 360.0 / (59 if odd else 60)
    yz = math.floor(131072 * ((lat % dlat) / dlat) + 0.5)
    rlat = dlat * (yz / 131072 + math.floor(lat / dlat))
    nl = max(oracle.calc_num_zones(rlat) - (1 if odd else 0), 1)
    dlon = 360.0 / nl
    xz = math.floor(131072 * ((lon % dlon) / dlon) + 0.5)
    return int(yz) & 0x1FFFF, int(xz) & 0x1FFFF


def test_split_pairs_get_a_position(gpu, oracle):
    """Receiver 0 hears only the even position frames of every aircraft, receiver 1 only the odd ones, both its
    identification: no per-receiver table has a position, so the fused view has none; one table fed the correlated list
    has the position the oracle's tracker gives for the time-merged list, and the wire carries each message once."""
    sps, shift = 1e-3, 700                                       # receiver 1's clock starts 700 samples later
    planes = [(0x4840D6, 52.25, 3.92), (0x40621D, -33.9, 151.2), (0x7C1234, 10.5, -75.3)]
    per = [[], []]
    for a, (icao, lat, lon) in enumerate(planes):
        for k in range(6):
            t = 2000 + 900 * k + 130 * a
            odd = k % 2
            fr = position_frame(oracle, icao, odd, *_cpr(oracle, lat + 0.001 * k, lon, odd))
            per[odd].append((t - shift * odd, fr, 0, 0xFF))
        ident = ident_frame(oracle, icao, [1 + a, 2, 3, 4, 5, 6, 7, 8])
        per[0].append((7600 + 130 * a, ident, 0, 0xFF))
        per[1].append((7600 + 130 * a + 1 - shift, ident, 0, 0xFF))                  # one sample later on receiver 1
    frames, counts = M.build(per)
    base = [0, shift]
    want = M.correlate(frames, counts, 2, base)
    assert len(want[0]) == len(frames) - len(planes) and want[0]["n_receivers"].max() == 2
    ot = oracle.tracker()
    for m in want[0]:
        ot.update(bytes(m["bytes"]), float(int(m["time"])) * sps)
    truth = sorted(ot.aircraft(), key=lambda s: s.icao)
    assert len(truth) == len(planes) and all(s.has_position for s in truth)
    with A.AdsbDemod(max_samples=4096, max_out=256) as d:
        with A.TrackBank(d, 2, max_frames=256, seconds_per_sample=sps) as bank:
            bank.update(frames, counts, base)
            fused, n_total, flags = bank.fuse()
            assert n_total == len(planes) == len(fused) and flags == 0
            assert (fused["has_position"] == 0).all() and (fused["n_receivers"] == 2).all()
        M.same(d.correlate_of(frames, counts, 2, base), want, "traffic")
        _, fdev, _, _ = d.correlated_device()
        n_msgs = len(want[0])
        with A.TrackTable(d, max_frames=256, seconds_per_sample=sps) as table:
            table.update_device(fdev, n_msgs, sample_base=0)
            recs, tflags = table.aircraft()
        assert tflags == 0 and [int(r["icao"]) for r in recs] == [s.icao for s in truth]
        for rec, s in zip(recs, truth):
            assert rec["has_position"] == 1 and rec["callsign"].decode() == s.callsign.decode()
            assert (rec["latitude"], rec["longitude"]) == pytest.approx((s.latitude, s.longitude), abs=1e-9)
            assert rec["last_contact"] == pytest.approx(s.last_contact, abs=1e-9)
        for fmt in (W.BEAST, W.AVR_MLAT):
            got = d.wire_of((fdev, n_msgs), format=fmt)
            stream, ends = W.encode(fmt, want[1])
            assert got[0] == stream and got[1].tolist() == ends.tolist()
            assert [p[-1] for p in W.parse(fmt, got[0])] == [bytes(m["bytes"]) for m in want[0]]   # each message once


# ---- 10: untouched paths; the argument checks that need a device -----------------------------------------------------------
def test_other_results_stay_as_they_are(gpu):
    cfg = A.synth_default(seed=5, slot_len=800)
    n = 40_000
    buf = np.concatenate([A.synth_fill_host(cfg, A.ADSB_SAMPLE_I8, c, 0, n) for c in range(2)])
    dev = _dev(buf)
    with A.AdsbDemod(max_samples=n, max_out=1 << 12, max_channels=2, host_staging=False) as d:
        d.demod_device_async(dev.data_ptr(), n, n_channels=2, channel_stride=n)
        frames, counts, total, flags = d.fetch()
        lv = d.levels()
        wire = d.wire("beast", signal=True)
        assert len(frames) > 40
        d.correlate(50, levels=True)
        fr2, lv2 = M.random_list(300, 4, seed=9)[0::2]
        d.correlate_of(fr2, [300, 0, 0, 0], 5, None, lv2)
        again, counts2, total2, flags2 = d.fetch()
        assert again.tobytes() == frames.tobytes() and list(counts2) == list(counts) and (total2, flags2) == (total, flags)
        assert d.levels().tobytes() == lv.tobytes()
        got = d.fetch_wire()
        assert got[0] == wire[0] and got[1].tolist() == wire[1].tolist()
    del dev


def test_argument_checks(ctx):
    L = _lib.load()
    h = ctx.handle
    fr, counts = M.build([[(5, K.KNOWN, 0, 0xFF), (9, K.KNOWN, 0, 0xFF)], [(6, K.KNOWN, 0, 0xFF)]])
    want = _check(ctx, fr, counts, 1, None, None, "before the rejected calls")
    good = _lib.AdsbCorrelateCfg(1, 0, 0)

    def call(cfg=C.byref(good), frames=fr.ctypes.data, n=3, cnt=(2, 1), R=2):
        arr = None if cnt is None else np.array(cnt, dtype=np.uint64)
        return L.adsb_correlate_of(h, cfg, frames, None, n, None if arr is None else arr.ctypes.data, R, None)

    assert call(cfg=None) == A.ADSB_E_ARG and call(frames=None) == A.ADSB_E_ARG and call(cnt=None) == A.ADSB_E_ARG
    assert call(R=0) == A.ADSB_E_ARG and call(cnt=[1] * 257, n=257, R=257) == A.ADSB_E_ARG
    assert call(cnt=(2, 2)) == A.ADSB_E_ARG and call(cnt=(1, 1)) == A.ADSB_E_ARG
    assert call(cnt=((1 << 64) - 1, 4)) == A.ADSB_E_ARG
    assert call(n=1 << 32, cnt=(1 << 32, 0)) == A.ADSB_E_CAPACITY
    M.same(ctx.fetch_correlated(), want, "rejected calls leave the result")
    # short capacities: the totals whatever they are, the first entries
    n_m, n_r = C.c_size_t(), C.c_size_t()
    msgs = np.zeros(1, dtype=M.MESSAGE_DTYPE)
    recs = np.zeros(2, dtype=M.RECEPTION_DTYPE)
    assert L.adsb_fetch_correlated(h, msgs.ctypes.data, 1, C.byref(n_m), recs.ctypes.data, 2, C.byref(n_r)) == A.ADSB_OK
    assert (n_m.value, n_r.value) == (2, 3) and msgs.tobytes() == want[0][:1].tobytes()
    assert recs.tobytes() == want[2][:2].tobytes()
    assert L.adsb_fetch_correlated(h, None, 1, None, None, 0, None) == A.ADSB_E_ARG
    assert call(frames=None, n=0, cnt=(0, 0)) == A.ADSB_OK
    assert [len(x) for x in ctx.fetch_correlated()] == [0, 0, 0]
