"""The scratch the C boundary keeps on a context (air_rs_amd/csrc/adsb_scratch.h) under reuse: levels_of, wire_of,
wire_in_of, correlate_of and multilaterate_of called in turn on one context with lists that grow, shrink and grow again,
in host and in device memory, and a block regrown while another feature's kernels still read it.  Every result is
compared with its CPU mirror: byte for byte, and for multilaterate under the rule of tests/test_mlat_host.py with no
message left out (every integer field equal, positions within its tolerance).  Each test takes a fresh context of the
same shape, so that every buffer starts empty and grows inside the test."""
import numpy as np
import pytest

import air_rs_amd as A
from tests import correlate_model as CM
from tests import levels_cases as LK
from tests import mlat_cases as K
from tests import wire_model as W
from tests.test_mlat_host import same_fixes

pytestmark = pytest.mark.gpu
NS = dict(seconds_per_tick=K.SPT_NS)
SIZES = (3, 300, 5, 301)
N_SAMPLES = 60_000
WINDOW = 40
BASE = [3 * r for r in range(5)]


@pytest.fixture
def ctx(gpu):
    with A.AdsbDemod(max_samples=1 << 16, max_out=1024) as d:
        yield d


def _dev(arr):
    import torch
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).reshape(-1)).cuda()


def _beast_of(frames, counts):
    """Receiver r's frames as Beast stream r -> (the streams end to end, their ends)."""
    streams, ends, at = [], [], 0
    for c in counts:
        streams.append(A.host_wire_encode(frames[at:at + int(c)])[0])
        at += int(c)
        ends.append(sum(len(s) for s in streams))
    return b"".join(streams), ends


@pytest.fixture(scope="module")
def cases(oracle):
    """Per list size: each feature's input and its mirror's answer, computed once."""
    iq = A.synth_fill_host(A.synth_default(seed=77, slot_len=450), A.ADSB_SAMPLE_I8, 0, 0, N_SAMPLES)
    rcv = K.receivers(6, seed=906)
    pos, emitted = K.emitters(oracle, max(SIZES), seed=907)
    full = K.build(rcv, pos, emitted)
    out = {"iq": iq, "rcv": rcv, "rx": full["rx"]}
    for n in SIZES:
        rng = np.random.default_rng(n)
        c = {}
        # levels: windows all over the buffer, the last of them one sample past its end
        c["lv_frames"] = LK.frame_list(np.sort(rng.integers(0, N_SAMPLES - 239, size=n - 1)).tolist() + [N_SAMPLES - 239])
        c["lv_want"] = A.host_frame_levels(iq, c["lv_frames"])
        c["w_frames"], c["w_levels"] = W.random_frames(n, seed=n), W.random_levels(n, seed=n + 1)
        c["w_want"] = A.host_wire_encode(c["w_frames"], c["w_levels"])
        c["wi_stream"] = c["w_want"][0]
        c["wi_want"] = A.host_wire_parse(c["wi_stream"], levels=True)
        c["c_frames"], c["c_counts"], c["c_levels"] = CM.random_list(n, 5, seed=100 + n, window=WINDOW)
        c["c_want"] = A.host_correlate(c["c_frames"], c["c_counts"], WINDOW, BASE, c["c_levels"])
        n_recs = int(full["msgs"]["first"][n]) if n < len(full["msgs"]) else len(full["recs"])
        c["m_msgs"], c["m_recs"] = full["msgs"][:n], full["recs"][:n_recs]
        c["m_want"] = A.host_multilaterate(rcv, c["m_msgs"], c["m_recs"], **NS)
        out[n] = c
    assert out[300]["lv_want"]["flags"].tolist() == [A.ADSB_LEVEL_VALID] * 299 + [0]
    assert int(out[301]["wi_want"].header["n_frames"]) == 301
    return out


def _same_wire_in(got, want, what):
    assert (got.levels is None) == (want.levels is None), what
    for name in ("frames", "rx", "counts", "consumed", "header") + (("levels",) if want.levels is not None else ()):
        assert getattr(got, name).tobytes() == getattr(want, name).tobytes(), (what, name)


def _same_mlat(got, want, what):
    same_fixes(got[0], want[0], None, 0.01, what)
    assert got[1].tobytes() == want[1].tobytes(), (what, "header")


def test_grow_shrink_grow_interleaved(ctx, cases):
    """Sizes 3, 300, 5, 301 with device lists, then again with host lists (whose device copies grow the same way), the
    five features in turn at each size: every regrow happens while the other features' blocks are alive."""
    dev_iq = _dev(cases["iq"])
    for where in ("device", "host"):
        for n in SIZES:
            c, what = cases[n], (where, n)
            held = {k: _dev(c[k]) for k in ("lv_frames", "w_frames", "w_levels", "c_frames", "c_levels", "m_msgs", "m_recs")}
            held["wi_stream"] = _dev(np.frombuffer(c["wi_stream"], dtype=np.uint8).copy())
            ptr = {k: t.data_ptr() for k, t in held.items()}
            on_dev = where == "device"

            frames = (ptr["lv_frames"], n) if on_dev else c["lv_frames"]
            got = ctx.levels_of(dev_iq.data_ptr(), N_SAMPLES, frames)
            assert got.tobytes() == c["lv_want"].tobytes(), (what, "levels_of")

            frames, levels = ((ptr["w_frames"], n), ptr["w_levels"]) if on_dev else (c["w_frames"], c["w_levels"])
            stream, ends = ctx.wire_of(frames, levels)
            assert stream == c["w_want"][0] and ends.tobytes() == c["w_want"][1].tobytes(), (what, "wire_of")

            data = (ptr["wi_stream"], len(c["wi_stream"])) if on_dev else c["wi_stream"]
            _same_wire_in(ctx.wire_in_of(data, levels=True), c["wi_want"], (what, "wire_in_of"))

            frames, levels = ((ptr["c_frames"], n), ptr["c_levels"]) if on_dev else (c["c_frames"], c["c_levels"])
            CM.same(ctx.correlate_of(frames, c["c_counts"], WINDOW, BASE, levels), c["c_want"], (what, "correlate_of"))

            msgs, recs = ((ptr["m_msgs"], n), (ptr["m_recs"], len(c["m_recs"]))) if on_dev else (c["m_msgs"], c["m_recs"])
            _same_mlat(ctx.multilaterate_of(cases["rcv"], msgs, recs, **NS), c["m_want"], (what, "multilaterate_of"))
            del held
    del dev_iq


def test_correlate_regrown_behind_multilaterate(ctx, oracle):
    """multilaterate reads correlate's block in place; the correlate call behind it needs a larger block.  The fixes are
    those of the first list, the correlate result is that of the second."""
    rcv = K.receivers(5, seed=936)
    pos, emitted = K.emitters(oracle, 60, seed=937)
    small, large = K.build(rcv, pos[:1], emitted[:1]), K.build(rcv, pos, emitted)
    assert len(small["frames"]) == 5 and len(large["frames"]) == 300
    window = 1_000_000
    want_small = A.host_correlate(small["frames"], small["counts"], window)
    want_large = A.host_correlate(large["frames"], large["counts"], window)
    want_fixes = A.host_multilaterate(rcv, want_small[0], want_small[2], **NS)
    ctx.correlate_of_async(small["frames"], small["counts"], window)
    ctx.multilaterate_async(rcv, **NS)
    ctx.correlate_of_async(large["frames"], large["counts"], window)
    _same_mlat(ctx.fetch_mlat(), want_fixes, "fixes of the 5-reception list")
    assert len(want_fixes[0]) == 1 and want_fixes[0]["flags"][0] & A.ADSB_MLAT_VALID
    CM.same(ctx.fetch_correlated(), want_large, "the 300-reception list")
    assert len(want_large[0]) == 60


def test_wire_in_regrown_behind_correlate(ctx):
    """correlate reads the parser's lists in place; the parse behind it needs a larger block."""
    streams = {}
    for n in (12, 300):
        frames, counts, _ = CM.random_list(n, 3, seed=200 + n, window=WINDOW)
        streams[n] = _beast_of(frames, counts)
    want_small, want_large = (A.host_wire_parse(*streams[n]) for n in (12, 300))
    assert int(want_small.header["n_frames"]) == 12 and int(want_large.header["n_frames"]) == 300
    want = A.host_correlate(want_small.frames, want_small.counts, WINDOW)
    ctx.wire_in_of_async(*streams[12])
    frames_dev = ctx.wire_in_device()[0]
    ctx.correlate_of_async((frames_dev, 12), want_small.counts, WINDOW)
    ctx.wire_in_of_async(*streams[300])
    CM.same(ctx.fetch_correlated(), want, "the small input's frames")
    assert 0 < len(want[0]) < 12
    _same_wire_in(ctx.fetch_wire_in(), want_large, "the larger input")
