"""Mode S replies on the device (adsb_modes_of, adsb_fetch_modes, adsb_modes_device): every output byte for byte equal to
the CPU mirror's and the independent model's (tests/modes_model.py), at every list and known_in size at which a kernel
takes another path -- T threads per workgroup, from adsb_debug_modes_geometry -- with lists in host and in device memory,
every AC and ID code, per-receiver counts, the cut property, and two runs against each other."""
import ctypes as C

import numpy as np
import pytest

import air_rs_amd as A
from air_rs_amd import _lib
from tests import modes_cases as K
from tests import modes_model as M
from tests.test_gpu_correlate import _dev, _read_device

pytestmark = pytest.mark.gpu


def _T():
    t = C.c_uint32()
    assert _lib.load().adsb_debug_modes_geometry(C.byref(t)) == A.ADSB_OK
    return t.value


@pytest.fixture(scope="module")
def ctx(gpu):
    with A.AdsbDemod(max_samples=1 << 16, max_out=1024) as d:
        yield d


@pytest.fixture(scope="module")
def big():
    """one list of about 70 000 frames with its model result, shared"""
    fr, pool = K.random_list(70_001, 99, n_addresses=3000)
    known = pool[::2].copy()
    return fr, known, M.modes(fr, known)


def _device_result(d, R):
    """the result read where modes_device() says it is, after the stream has drained"""
    got = d.fetch_modes()                                                                      # waits
    recs, known, sq, sqc, hdr = d.modes_device()
    h = _read_device(hdr, np.dtype("<u8"), 8)
    assert h.tolist() == [int(got[4][k]) for k in M.HEADER_FIELDS] and (sqc is not None) == bool(R)
    return (_read_device(recs, M.REC_DTYPE, int(h[0])), _read_device(known, np.dtype("<u4"), int(h[6])),
            _read_device(sq, M.FRAME_DTYPE, int(h[7])), _read_device(sqc, np.dtype("<u8"), R) if R else None, got[4])


def _check(d, fr, known, counts=None, want=None, what=""):
    """device == mirror == model; returns the model's result"""
    want = M.modes(fr, known, counts) if want is None else want
    M.same(d.modes_of(fr, counts, known), want, (what, "device"))
    M.same(_device_result(d, 0 if counts is None else len(counts)), want, (what, "device arrays"))
    M.same(A.host_modes(fr, counts, known), want, (what, "mirror"))
    return want


def test_state_before_the_first_call(gpu):
    L = _lib.load()
    with A.AdsbDemod(max_samples=1 << 16, max_out=64) as d:
        assert L.adsb_fetch_modes(d.handle, None, 0, None, 0, None, 0, None, 0, None) == A.ADSB_E_STATE
        assert L.adsb_modes_device(d.handle, None, None, None, None, None) == A.ADSB_E_STATE
        assert L.adsb_modes_of(None, None, 0, None, 0, None, 0) == A.ADSB_E_ARG
        d.modes_of(M.frame_list([K.KNOWN_FRAME]))
        assert L.adsb_fetch_modes(d.handle, None, 0, None, 0, None, 0, None, 0, None) == A.ADSB_OK


@pytest.mark.parametrize("case", K.all_cases(), ids=[c[0] for c in K.all_cases()])
def test_case_lists(ctx, case):
    name, fr, known = case
    _check(ctx, fr, known, what=name)


def test_list_and_known_in_sizes(ctx):
    t = _T()
    fr, pool = K.random_list(2 * t + 1, 5, n_addresses=2 * t + 40)
    assert len(pool) > t + 1
    seen = set()
    for n in (0, 1, t - 1, t, t + 1, 2 * t + 1):
        for nk in (0, 1, t, t + 1):
            want = _check(ctx, fr[:n], pool[:nk], what=(n, nk))
            seen |= set(want["recs"]["kind"].tolist())
    assert seen == {M.SELF, M.KNOWN, M.UNKNOWN, M.PARITY, M.UNSUPPORTED}


def test_the_large_list_in_host_and_device_memory_twice(ctx, big):
    fr, known, want = big
    assert want["header"]["n_known"] > 5000 and want["header"]["n_squitters"] > 5000 and want["header"]["n_unknown"] > 5000
    first = ctx.modes_of(fr, None, known)
    M.same(first, want, "host lists")
    dev_fr, dev_known = _dev(fr), _dev(known)
    second = ctx.modes_of((dev_fr.data_ptr(), len(fr)), None, (dev_known.data_ptr(), len(known)))
    M.same(second, want, "device lists")
    third = ctx.modes_of((dev_fr.data_ptr(), len(fr)), None, known)                              # mixed
    for a, b, c in zip(first[:3], second[:3], third[:3]):
        assert a.tobytes() == b.tobytes() == c.tobytes()                                         # run to run: the same bytes
    M.same(_device_result(ctx, 0), want, "device arrays")
    del dev_fr, dev_known


def test_self_before_and_after_across_a_block_boundary(ctx):
    t = _T()
    filler = M.reply(5, K.C)
    for at in (t - 1, t):                                            # the SELF frame at index `at`: pairs (t-1, t), (t, t+1)
        for lead in (0, 1):
            msgs = [filler] * (at - 1 + lead) + ([M.reply(4, K.A)] if not lead else []) + [M.all_call(K.A), M.reply(4, K.A)]
            msgs += [filler] * 5
            s = msgs.index(M.all_call(K.A))
            assert s == at
            want = _check(ctx, M.frame_list(msgs), [], what=(at, lead))
            assert want["recs"]["kind"][s + 1] == M.KNOWN and (lead or want["recs"]["kind"][s - 1] == M.UNKNOWN)


def test_every_ac_and_id_code(ctx):
    """all 8192 values of the 13-bit field under DF0/4/16/20 (AC) and DF5/21 (ID), addresses known: one call"""
    f = np.arange(8192, dtype=np.uint32)
    rows = []
    for df in (0, 4, 16, 20, 5, 21):
        b = np.zeros((8192, 14), dtype=np.uint8)
        b[:, 0], b[:, 1] = df << 3 | 5, 0xA7
        b[:, 2], b[:, 3] = 0xE0 | f >> 8, f & 0xFF
        k = 4 if df < 16 else 11
        p = M.crc24_many(b[:, :k]) ^ np.uint32(K.A)
        b[:, k], b[:, k + 1], b[:, k + 2] = p >> 16, (p >> 8) & 0xFF, p & 0xFF
        rows.append(b)
    fr = np.zeros(6 * 8192, dtype=M.FRAME_DTYPE)
    fr["bytes"], fr["fixed_bit"] = np.concatenate(rows), 0xFF
    want = _check(ctx, fr, [K.A], what="AC and ID")
    recs = want["recs"]
    assert (recs["kind"] == M.KNOWN).all() and (recs["address"] == K.A).all()
    for k in range(4):                                               # 1280 Gillham + 2048 25 ft codes have an altitude
        part = recs[k * 8192:(k + 1) * 8192]
        assert ((part["flags"] & M.ALT) != 0).sum() == 1280 + 2048 and ((part["flags"] & M.ALT_METRIC) != 0).sum() == 4096
        assert part["altitude_ft"].min() == -1200 and part["altitude_ft"].max() == 126700
    assert len(set(recs[4 * 8192:]["squawk"].tolist())) == 4096 and (recs[4 * 8192:]["flags"] & M.SQUAWK != 0).all()


@pytest.mark.parametrize("R", [1, 3, 256])
def test_squitter_counts(ctx, big, R):
    fr, known = big[0][:5000], big[1]
    edges = np.sort(np.random.default_rng(R).integers(0, len(fr) + 1, size=R - 1))
    counts = np.diff(np.concatenate([[0], edges, [len(fr)]])).astype(np.uint64)
    want = _check(ctx, fr, known, counts, what=R)
    got = ctx.fetch_modes()
    assert int(got[3].sum()) == int(got[4]["n_squitters"]) == want["header"]["n_squitters"] > 300


def test_cut_property_on_the_device(ctx):
    t = _T()
    fr, pool = K.random_list(3 * t + 7, 31)
    known = pool[::2].copy()
    whole = ctx.modes_of(fr, None, known)
    late = (whole[0]["kind"] == M.KNOWN) & ~np.isin(whole[0]["address"], known)
    assert late.sum() > 20                                           # addresses learnt inside the list
    cuts = [t - 1, t, t + 1] + sorted(int(x) for x in np.random.default_rng(3).integers(0, len(fr) + 1, size=20))
    for cut in cuts:
        one = ctx.modes_of(fr[:cut], None, known)
        # known_out stays on the device: the next call takes it where it lies
        two = ctx.modes_of(fr[cut:], None, (ctx.modes_device()[1], len(one[1])))
        assert np.concatenate([one[0], two[0]]).tobytes() == whole[0].tobytes(), cut
        assert two[1].tolist() == whole[1].tolist() and np.concatenate([one[2], two[2]]).tobytes() == whole[2].tobytes(), cut
        three = ctx.modes_of(fr[cut:], None, one[1])                 # and through the host
        assert all(a.tobytes() == b.tobytes() for a, b in zip(two[:3], three[:3])), cut


def test_argument_checks_and_short_fetches(ctx):
    L, h = _lib.load(), ctx.handle
    fr = M.frame_list([K.KNOWN_FRAME, M.reply(4, K.A), M.squitter(K.B)])
    want = _check(ctx, fr, [K.B], [2, 1], what="before the rejected calls")
    bad = np.array([5, 5], dtype=np.uint32)
    cnt = np.array([1, 1], dtype=np.uint64)
    assert L.adsb_modes_of(h, None, 3, None, 0, None, 0) == A.ADSB_E_ARG
    assert L.adsb_modes_of(h, fr.ctypes.data, 3, None, 0, bad.ctypes.data, 2) == A.ADSB_E_ARG      # a host known_in is checked
    assert L.adsb_modes_of(h, fr.ctypes.data, 3, None, 0, None, 1) == A.ADSB_E_ARG
    assert L.adsb_modes_of(h, fr.ctypes.data, 3, cnt.ctypes.data, 2, None, 0) == A.ADSB_E_ARG      # counts sum to 2
    assert L.adsb_modes_of(h, fr.ctypes.data, 3, cnt.ctypes.data, 0, None, 0) == A.ADSB_E_ARG
    assert L.adsb_modes_of(h, fr.ctypes.data, 1 << 32, None, 0, None, 0) == A.ADSB_E_CAPACITY
    M.same(ctx.fetch_modes(), want, "rejected calls leave the result")
    recs, hdr = np.zeros(2, dtype=M.REC_DTYPE), _lib.AdsbModesHeader()
    one = np.zeros(1, dtype=np.uint64)
    assert L.adsb_fetch_modes(h, recs.ctypes.data, 2, None, 0, None, 0, one.ctypes.data, 1, C.byref(hdr)) == A.ADSB_OK
    assert recs.tobytes() == want["recs"][:2].tobytes() and (hdr.n, hdr.n_squitters, int(one[0])) == (3, 2, 1)
    assert L.adsb_fetch_modes(h, None, 2, None, 0, None, 0, None, 0, None) == A.ADSB_E_ARG
    assert L.adsb_fetch_modes(h, None, 0, None, 0, None, 0, one.ctypes.data, 3, None) == A.ADSB_E_ARG  # more receivers than given


def test_other_results_stay_as_they_are(gpu):
    """a ctx that never calls the stage is the ctx it was; one that does keeps every other result"""
    cfg = A.synth_default(seed=5, slot_len=800)
    n = 40_000
    dev = _dev(np.concatenate([A.synth_fill_host(cfg, A.ADSB_SAMPLE_I8, c, 0, n) for c in range(2)]))
    with A.AdsbDemod(max_samples=n, max_out=1 << 12, max_channels=2, host_staging=False) as d:
        d.demod_device_async(dev.data_ptr(), n, n_channels=2, channel_stride=n)
        frames, counts, total, flags = d.fetch()
        lv = d.levels()
        wire = d.wire("beast", signal=True)
        corr = d.correlate(50, levels=True)
        parsed = d.wire_in_of(wire[0], levels=True)
        assert len(frames) > 40
        got = d.modes_of(frames, counts)                             # the demodulator's own list
        assert (got[0]["kind"] == M.SELF).sum() > 40 and int(got[3].sum()) == len(got[2]) == int(got[4]["n_squitters"])
        M.same(got, M.modes(frames, (), counts), "the launch's list")
        d.modes_of(K.random_list(5000, 1)[0])                        # grows the buffers
        again, counts2, total2, flags2 = d.fetch()
        assert again.tobytes() == frames.tobytes() and list(counts2) == list(counts) and (total2, flags2) == (total, flags)
        assert d.levels().tobytes() == lv.tobytes()
        back = d.fetch_wire()
        assert back[0] == wire[0] and back[1].tolist() == wire[1].tolist()
        assert all(x.tobytes() == y.tobytes() for x, y in zip(d.fetch_correlated(), corr))
        assert all(x.tobytes() == y.tobytes() for x, y in zip(d.fetch_wire_in()[:2], parsed[:2]))
    del dev
