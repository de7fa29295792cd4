"""The CS16 scan (demod_tiles<ADSB_SAMPLE_I16>, adsb_kernels.hip) where it decides on single magnitudes, bit-exact against the CPU
oracle through the C ABI: the two gates a tile chooses between (the packed f16 three-input gate below 31744, the integer gate
otherwise), the choice itself (a per-wave ballot over the samples each wave loaded, the halo sweep included), ties after the
root's truncation in both gates, and the CS16 slicer on the same ties.

The buffers are hand-built from real (I, Q) samples (tests/cs16_cases.py; tests/test_cs16_cases.py checks the builders on the CPU):
every planted window is a whole valid DF17 frame, so a gate or slicer verdict that differs from the reference adds or removes
a frame.  The number of planted frames the reference returns is asserted first, from the model, so the intended path is the
one taken.  Both launch paths: every buffer is at most 32 tiles, so ADSB_SMALL_PATH=1 really takes demod_small."""
import numpy as np
import pytest

import air_rs_amd as A
from tests import cs16_cases as C
from tests import survivor_cases as S

pytestmark = pytest.mark.gpu
_REF = {}


def _want(oracle, b):
    """the oracle's list of one buffer; computed once, shared by every test, never written to"""
    if b.name not in _REF:
        rc, want, found = oracle.process_buffer(b.iq, max_out=1 << 12)
        assert rc == 0 and found == len(want)
        _REF[b.name] = want
    return _REF[b.name]


def _eq(got, want):
    assert len(got) == len(want), (len(got), len(want))
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (bad[:5], got[bad[:3]], want[bad[:3]])


def _run(oracle, monkeypatch, small, bufs, n_pass=None):
    monkeypatch.setenv("ADSB_SMALL_PATH", small)
    with A.AdsbDemod(sample_type=A.ADSB_SAMPLE_I16, max_samples=max(b.n for b in bufs), max_out=1 << 12) as d:
        for b in bufs:
            assert b.n <= 262144
            want = _want(oracle, b)
            planted = sum(w.ok for _, w in b.plants)
            assert len(want) == planted and (want["offset"] == b.expected()["offset"]).all(), (b.name, len(want), planted)
            assert 0 < planted and (n_pass is None or n_pass(b, planted)), (b.name, planted)
            frames, flags = d.demod(b.iq)
            assert flags == 0, (b.name, flags)
            _eq(frames, want)


@pytest.mark.parametrize("small", ["1", "0"])
def test_root_ties_in_the_f16_gate(gpu, oracle, monkeypatch, small):
    """every boundary root below 31744 -- the first classes, the f16 denormal | normal edge, every exponent edge, 31742 | 31743 --
    as a tie (both orders of I^2 + Q^2), one class below and one class above, in the preamble and in the DF17 part, at all
    four positions of a 16-byte load and in both runs of a lane; every tile and its halo below 31744"""
    bufs = C.built(oracle)["f16"]
    assert all(b.tile_max(t) < C.F16_LIMIT for b in bufs for t in range(b.tiles()))
    # (three relations of four pass: a buffer that lost its failing windows, or its passing ones, would show here)
    _run(oracle, monkeypatch, small, bufs, lambda b, k: len(b.plants) // 2 < k < len(b.plants))


@pytest.mark.parametrize("small", ["1", "0"])
def test_root_ties_in_the_integer_gate(gpu, oracle, monkeypatch, small):
    """the same four relations where a magnitude is 31744 or more (infinity, NaN and negative f16 patterns, up to the corners
    of the i16 range): every tile holds such a sample"""
    bufs = C.built(oracle)["integer"]
    assert all(b.tile_max(t, halo=False) >= C.F16_LIMIT for b in bufs for t in range(b.tiles()))
    _run(oracle, monkeypatch, small, bufs, lambda b, k: len(b.plants) // 2 < k < len(b.plants))


@pytest.mark.parametrize("small", ["1", "0"])
def test_one_big_sample_switches_the_whole_tile(gpu, oracle, monkeypatch, small):
    """windows the reference rejects and the f16 gate would pass (a negative pattern among the gaps, a NaN pattern among the
    pulses), in a tile whose only sample of 31744 or more is that one: in the share of each wave, at the tile's first and
    last sample, and in the halo alone.  Only the control frames of the spare tiles (and the windows whose big sample no gate
    reads) come back."""
    bufs = C.built(oracle)["gate choice"]
    for b in bufs:
        for t, (name, p) in b.notes.items():
            span = b.mag[t * C.TILE:(t + 1) * C.TILE + (C.HALO if t % 2 == 0 else 0)]
            assert list(np.nonzero(span >= C.F16_LIMIT)[0]) == [p], (b.name, name)
    _run(oracle, monkeypatch, small, bufs,
         lambda b, k: k == len(b.plants) // 2 + sum(w.name.startswith("last sample") for _, w in b.plants))


@pytest.mark.parametrize("small", ["1", "0"])
def test_slicer_ties_after_truncation(gpu, oracle, monkeypatch, small):
    """valid frames whose every 0 bit is a tie of two different I^2 + Q^2 in one root class (larger first), and their mirror
    images in one-class steps: all of them come back"""
    _run(oracle, monkeypatch, small, C.built(oracle)["slicer"], lambda b, k: k == len(b.plants))


@pytest.mark.parametrize("small", ["1", "0"])
def test_three_channels_mixed_gates(gpu, oracle, monkeypatch, small):
    """one launch of three channels: f16-gate tiles only, integer-gate tiles only, the two alternating; a ragged last tile each
    with a decision window at the last offset the reference looks at; padding of full-scale samples between the channels"""
    import torch
    monkeypatch.setenv("ADSB_SMALL_PATH", small)
    bufs = C.built(oracle)["channels"]
    n, nch = bufs[0].n, len(bufs)
    assert nch == 3 and all(b.n == n for b in bufs) and (n - S.WINDOW) % C.TILE != 0
    stride = (n + 7) // 8 * 8 + 8  # (a stride is a multiple of 8 samples)
    host = np.full((nch, stride, 2), 32767, dtype=np.int16)  # padding between channels must never be looked at
    wants = []
    for c, b in enumerate(bufs):
        want = _want(oracle, b)
        planted = sum(w.ok for _, w in b.plants)
        assert len(want) == planted and 24 < planted < len(b.plants) - 8, (b.name, len(want), planted)
        assert want["offset"][-1] == n - S.WINDOW - 1 and (want["offset"] == b.expected()["offset"]).all()
        for t, kind in b.notes.items():
            assert (b.tile_max(t) < C.F16_LIMIT) if kind == "f" else (b.tile_max(t, halo=False) >= C.F16_LIMIT), (b.name, t)
        host[c, :n] = b.iq
        wants.append(want)
    with A.AdsbDemod(sample_type=A.ADSB_SAMPLE_I16, max_samples=n, max_out=1 << 12, max_channels=nch, host_staging=False) as d:
        t = torch.from_numpy(host).cuda()
        d.demod_device_async(t.data_ptr(), n, nch, stride)
        frames, got_counts, total, flags = d.fetch(n_channels=nch)
        assert flags == 0 and total == len(frames) == sum(len(w) for w in wants)
        pos = 0
        for c in range(nch):
            assert got_counts[c] == len(wants[c])
            _eq(frames[pos:pos + len(wants[c])], wants[c])
            pos += len(wants[c])
