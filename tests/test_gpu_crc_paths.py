"""Every CRC syndrome class (tests/crc_cases.py) through every path of the device that decides it, bit-exact against the CPU
oracle through the C ABI.

The verdict on s = CRC24(data) ^ crc_field is computed twice in adsb_kernels.hip: finish_record (byte table, binary search
over the 88 sorted syndromes, flip by byte and dword), reached from finish_block's one lane per survivor (tiles of at most 16),
from finish_big_tile's whole wave (ranked up to 64 survivors, ordered chunks of 64 above) and from demod_small; and
count_candidate (XOR of the per-bit table, a match by lanes 0..10), which only COUNTS the frames of a tile that lost its slots,
for the host to plan the re-run's output positions from.  Each layout puts all classes -- clean, every repairable data bit, the
DF17 ties, every CRC-field bit, the binary search's edges, aliased repairs, stubs -- into tiles of one survivor band, repaired,
dropped and clean frames side by side, and the oracle's own figures for every class and the band of every tile are asserted
before the device is asked, so the intended path is certainly the one taken."""
import numpy as np
import pytest

import air_rs_amd as A
from tests import crc_cases as C
from tests import survivor_cases as S

pytestmark = pytest.mark.gpu
TILES = {A.ADSB_SAMPLE_I8: 16384, A.ADSB_SAMPLE_I16: 8192}
DTYPES = {A.ADSB_SAMPLE_I8: np.int8, A.ADSB_SAMPLE_I16: np.int16}
STS = [A.ADSB_SAMPLE_I8, A.ADSB_SAMPLE_I16]
_REF = {}


def _case(oracle, st, path, n=None):
    """(iq, the oracle's list, Layout) of one layout (n: padded with background to that length); computed once, shared by every
    test, never written to.  The class figures and the bands are asserted here, on the oracle."""
    if (st, path, n) not in _REF:
        c = C.cases(oracle, TILES[st], path)
        mag = C.magnitudes(c, n)
        iq = S.to_iq(mag, DTYPES[st])
        rc, want, found = oracle.process_buffer(iq, max_out=1 << 12)
        assert rc == 0 and found == len(want)
        C.check_figures(c, want)
        C.check_bands(c, mag)
        C.check_mix(c)
        assert S.gate(mag)[len(c.band) * c.tile:].sum() == 0  # (padding: background only)
        iq.setflags(write=False)
        _REF[(st, path, n)] = (iq, want, c)
    return _REF[(st, path, n)]


def _eq(got, want):
    assert len(got) == len(want), (len(got), len(want))
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (bad[:5], got[bad[:3]], want[bad[:3]])


def _max_samples(oracle, st):
    return max(C.cases(oracle, TILES[st], p).n_samples for p in C.PATHS)


@pytest.mark.parametrize("path", C.PATHS)
@pytest.mark.parametrize("small", ["1", "0"])
@pytest.mark.parametrize("st", STS)
def test_plain_launch(gpu, oracle, monkeypatch, st, small, path):
    """finish_record from finish_block (sparse), finish_big_tile (quota, pool: ranked; dense: chunks of 64) and demod_small"""
    monkeypatch.setenv("ADSB_SMALL_PATH", small)
    iq, want, c = _case(oracle, st, path)
    with A.AdsbDemod(sample_type=st, max_samples=c.n_samples, max_out=1 << 12) as d:
        frames, flags = d.demod(iq)
        assert flags == 0
        _eq(frames, want)


@pytest.mark.parametrize("path", ["pool", "dense"])
@pytest.mark.parametrize("small", ["1", "0"])
@pytest.mark.parametrize("st", STS)
def test_cold_count_then_rerun(gpu, oracle, monkeypatch, st, small, path):
    """every tile loses its slots, count_candidate counts its frames, the host plans the re-run's positions from the counts and
    finish_record decides again: the same list, no flag -- a frame the two disagree on would leave a hole or an overlap"""
    monkeypatch.setenv("ADSB_SMALL_PATH", small)
    iq, want, c = _case(oracle, st, path)
    with A.AdsbDemod(sample_type=st, max_samples=c.n_samples, max_out=1 << 12) as d:
        d.pool_limit(True)
        frames, flags = d.demod(iq)
        d.pool_limit(False)
        assert flags == 0
        _eq(frames, want)
        frames, flags = d.demod(iq)  # the knob left no trace
        assert flags == 0
        _eq(frames, want)


@pytest.mark.parametrize("path", ["pool", "dense"])
@pytest.mark.parametrize("small", ["1", "0"])
@pytest.mark.parametrize("st", STS)
def test_cold_count_with_a_cut_list(gpu, oracle, monkeypatch, st, small, path):
    """max_out ends the list INSIDE a re-planned tile (the third, and the first): the first max_out frames, truncated, complete"""
    monkeypatch.setenv("ADSB_SMALL_PATH", small)
    iq, want, c = _case(oracle, st, path)
    per_tile = C.valid_per_tile(want, c.tile, len(c.band))
    for t in (2, 0):
        max_out = int(per_tile[:t].sum() + per_tile[t] // 2)
        assert per_tile[:t].sum() < max_out < per_tile[:t + 1].sum()
        # (the context's own max_out: the device and the host's plan stop there, not only the copy to the caller)
        with A.AdsbDemod(sample_type=st, max_samples=c.n_samples, max_out=max_out) as d:
            d.pool_limit(True)
            frames, flags = d.demod(iq)
            d.pool_limit(False)
            assert flags & A.ADSB_FLAG_TRUNCATED and not (flags & A.ADSB_FLAG_INCOMPLETE), (t, flags)
            _eq(frames, want[:max_out])


@pytest.mark.parametrize("small", ["1", "0"])
@pytest.mark.parametrize("st", STS)
def test_three_channels(gpu, oracle, monkeypatch, st, small):
    """sparse, pool and dense as channels 0..2 of one launch with the pool off: the sparse channel keeps its slots, the other two
    are counted and re-run; per-channel counts and lists"""
    import torch
    monkeypatch.setenv("ADSB_SMALL_PATH", small)
    paths = ("sparse", "pool", "dense")
    n = _max_samples(oracle, st)
    stride = n + 304  # (a multiple of 8 samples, larger than n)
    assert n % 8 == 0
    host = np.full((len(paths), stride, 2), 77, dtype=DTYPES[st])  # padding between channels must never be looked at
    wants = []
    for ch, path in enumerate(paths):
        iq, want, _ = _case(oracle, st, path, n)
        host[ch, :n] = iq
        wants.append(want)
    with A.AdsbDemod(sample_type=st, max_samples=n, max_out=1 << 12, max_channels=len(paths), host_staging=False) as d:
        t = torch.from_numpy(host).cuda()
        d.pool_limit(True)
        d.demod_device_async(t.data_ptr(), n, len(paths), stride)
        frames, got_counts, total, flags = d.fetch(n_channels=len(paths))
        d.pool_limit(False)
        assert flags == 0 and total == len(frames) == sum(len(w) for w in wants)
        pos = 0
        for ch in range(len(paths)):
            assert got_counts[ch] == len(wants[ch])
            _eq(frames[pos:pos + len(wants[ch])], wants[ch])
            pos += len(wants[ch])
