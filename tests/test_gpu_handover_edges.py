"""The survivor hand-over's count thresholds (hand_over, adsb_kernels.hip), one tile at a time.

With constant IQ every offset passes the gate and decodes to an all-zero frame, so a buffer of 240 + k constant samples puts
exactly k survivors into one ragged tile, and TILE + 240 + k puts a full dense tile in front of it.  k walks over the edges
of the hand-over: 32 | 33 the tile's own quota of slots against the pool, 64 | 65 the unordered list against the ordered
compaction of the bitmap, 128 | 129 one chunk of the list against two, 300 a third chunk.  Both sample types (their tiles
and bitmap words differ), both launch paths, bit-exact against the CPU oracle -- whose own count is asserted first, so the
intended path is certainly the one taken."""
import numpy as np
import pytest

import air_rs_amd as A

pytestmark = pytest.mark.gpu
KS = (1, 32, 33, 64, 65, 128, 129, 300)
TILES = {A.ADSB_SAMPLE_I8: 16384, A.ADSB_SAMPLE_I16: 8192}
DTYPES = {A.ADSB_SAMPLE_I8: np.int8, A.ADSB_SAMPLE_I16: np.int16}
_REF = {}


def _value(st, k):
    if k == 129:  # full-scale negative (CS16: magnitudes beyond the ordered f16 patterns, the integer gate)
        return (-128, -128) if st == A.ADSB_SAMPLE_I8 else (-32768, -32768)
    return (3, 4)


def _case(oracle, st, n, k):
    """(iq, the oracle's list) for n constant samples; computed once, shared by every test, never written to"""
    key = (st, n)
    if key not in _REF:
        iq = np.empty((n, 2), dtype=DTYPES[st])
        iq[:] = _value(st, k)
        rc, want, found = oracle.process_buffer(iq, max_out=1 << 15)
        assert rc == 0 and found == len(want)
        iq.setflags(write=False)
        _REF[key] = (iq, want)
    return _REF[key]


def _eq(got, want):
    assert len(got) == len(want), (len(got), len(want))
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (bad[:5], got[bad[:3]], want[bad[:3]])


@pytest.mark.parametrize("small", ["1", "0"])
@pytest.mark.parametrize("st", [A.ADSB_SAMPLE_I8, A.ADSB_SAMPLE_I16])
def test_survivor_counts_at_the_hand_over_edges(gpu, oracle, monkeypatch, st, small):
    tile = TILES[st]
    monkeypatch.setenv("ADSB_SMALL_PATH", small)
    with A.AdsbDemod(sample_type=st, max_samples=tile + 240 + max(KS), max_out=1 << 15) as d:
        for k in KS:
            for dense_tiles in (0, 1):  # the ragged tile alone; a full dense tile in front of it
                iq, want = _case(oracle, st, dense_tiles * tile + 240 + k, k)
                assert len(want) == dense_tiles * tile + k
                assert (want["offset"] == np.arange(len(want))).all() and not want["bytes"].any()
                frames, flags = d.demod(iq)
                assert flags == 0, (k, dense_tiles, flags)
                _eq(frames, want)


@pytest.mark.parametrize("st", [A.ADSB_SAMPLE_I8, A.ADSB_SAMPLE_I16])
def test_tiles_without_slots_are_counted_in_place_and_re_run(gpu, oracle, monkeypatch, st):
    """adsb_debug_pool_limit: a tile over its quota gets no slots, counts its frames in place (kNoBase) and the host
    re-runs it: no flag, the same list -- just past the unordered list (one chunk) and at three chunks"""
    tile = TILES[st]
    for small in ("1", "0"):
        monkeypatch.setenv("ADSB_SMALL_PATH", small)
        with A.AdsbDemod(sample_type=st, max_samples=tile + 240 + max(KS), max_out=1 << 15) as d:
            d.pool_limit(True)
            for k in (65, 300):
                for dense_tiles in (0, 1):
                    iq, want = _case(oracle, st, dense_tiles * tile + 240 + k, k)
                    assert len(want) == dense_tiles * tile + k
                    frames, flags = d.demod(iq)
                    assert flags == 0, (k, dense_tiles, flags)
                    _eq(frames, want)
            d.pool_limit(False)
