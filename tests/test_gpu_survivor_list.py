"""The per-tile work on the gate's few survivors (gate_phase's cold block with its append to the survivor list, and hand_over,
adsb_kernels.hip), one small tile set at a time, bit-exact against the CPU oracle through the C ABI.

A survivor is appended to the list by the lane that found it, inside the cold block (offsets at or beyond n_valid are dropped
there: the `past` cases below), and hand_over takes the survivor count and the wave number as scalars, so whole waves leave it
early.  The buffers are hand-built PPM (tests/survivor_cases.py) whose survivor count per tile is asserted
first, from a model of the reference gate, so the intended path is certainly the one taken: tile edges (offsets at or beyond
n_valid, frames at offset 0, at the A/B run boundary and among a tile's last offsets), survivor counts around every switch
(4 | 8 | 9 | 16 the waves that slice, 32 | 40 the tile's own slots and the pool, 64 | 65 the list and the bitmap, and tiles that
lose their slots), DF17 windows that fail on their first three bit pairs only or on the last two only, ties included.  Both sample types, both launch paths, and three
channels with a ragged last tile each."""
import numpy as np
import pytest

import air_rs_amd as A
from tests import survivor_cases as S

pytestmark = pytest.mark.gpu
TILES = {A.ADSB_SAMPLE_I8: 16384, A.ADSB_SAMPLE_I16: 8192}
DTYPES = {A.ADSB_SAMPLE_I8: np.int8, A.ADSB_SAMPLE_I16: np.int16}
STS = [A.ADSB_SAMPLE_I8, A.ADSB_SAMPLE_I16]
EDGES = (-241, -240, -239, 0, 239, 240, 241)
COUNTS = (0, 1, 4, 8, 9, 16, 32, 40, 64, 65)
_REF = {}


def _case(oracle, st, key, make):
    """(iq, the oracle's list, survivors per tile) of one buffer; computed once, shared by every test, never written to"""
    if (st, key) not in _REF:
        n, plants = make()
        mag = S.build(n, plants)
        iq = S.to_iq(mag, DTYPES[st])
        rc, want, found = oracle.process_buffer(iq, max_out=1 << 12)
        assert rc == 0 and found == len(want)
        iq.setflags(write=False)
        _REF[(st, key)] = (iq, want, S.survivors_per_tile(mag, TILES[st]))
    return _REF[(st, key)]


def _eq(got, want):
    assert len(got) == len(want), (len(got), len(want))
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (bad[:5], got[bad[:3]], want[bad[:3]])


def _edge(oracle, st, d, past):
    """one full tile + halo with d samples added: frames at offset 0, at the A/B run boundary (its last offset of run A for odd
    d, its first of run B for even d), in the last offsets of the tile, and at the last offset the reference looks at -- or
    (`past`) one beyond it, where the whole frame is still inside the buffer and the reference does not look"""
    tile = TILES[st]
    n = tile + S.WINDOW + d
    last = n - S.WINDOW - 1
    fb = lambda i: S.ppm(S.frame_bytes(oracle, 20 + i))
    plants = [(0, fb(0)), (tile // 2 - (d & 1), fb(1)), (last + past, fb(2))]
    if d > 0:
        plants.append((tile - 100, fb(3)))  # among the tile's last offsets; the frame runs on into the next tile's samples
    return n, plants


@pytest.mark.parametrize("small", ["1", "0"])
@pytest.mark.parametrize("st", STS)
def test_tile_edges_and_the_last_valid_offset(gpu, oracle, monkeypatch, st, small):
    tile = TILES[st]
    monkeypatch.setenv("ADSB_SMALL_PATH", small)
    with A.AdsbDemod(sample_type=st, max_samples=tile + 2 * S.WINDOW + 8, max_out=1 << 12) as d:
        for e in EDGES:
            for past in (0, 1):
                iq, want, counts = _case(oracle, st, ("edge", e, past), lambda: _edge(oracle, st, e, past))
                n_planted = 3 + (e > 0) - past
                assert sum(counts) == len(want) == n_planted, (e, past, counts, len(want))
                frames, flags = d.demod(iq)
                assert flags == 0, (e, past, flags)
                _eq(frames, want)


def _counted(oracle, st, k):
    tile = TILES[st]
    return 2 * tile + S.WINDOW + 100, S.tile_with(oracle, 0, k, k) + S.tile_with(oracle, tile, 1, 90)


@pytest.mark.parametrize("small", ["1", "0"])
@pytest.mark.parametrize("st", STS)
def test_exact_survivor_counts_per_tile(gpu, oracle, monkeypatch, st, small):
    """k survivors in the first tile (whole frames, then stubs that only take a slot), one in the second, a ragged third"""
    monkeypatch.setenv("ADSB_SMALL_PATH", small)
    with A.AdsbDemod(sample_type=st, max_samples=2 * TILES[st] + S.WINDOW + 100, max_out=1 << 12) as d:
        for k in COUNTS:
            iq, want, counts = _case(oracle, st, ("count", k), lambda: _counted(oracle, st, k))
            assert counts == [k, 1, 0] and len(want) == min(k, 16) + 1, (k, counts, len(want))
            frames, flags = d.demod(iq)
            assert flags == 0, (k, flags)
            _eq(frames, want)
        d.pool_limit(True)  # a tile over its quota gets no slots, counts its frames in place, and the host re-runs it
        for k in (40, 65):
            iq, want, counts = _case(oracle, st, ("count", k), lambda: _counted(oracle, st, k))
            frames, flags = d.demod(iq)
            assert flags == 0, (k, flags)
            _eq(frames, want)
        d.pool_limit(False)


@pytest.mark.parametrize("small", ["1", "0"])
@pytest.mark.parametrize("st", STS)
def test_df17_windows_that_fail_on_some_bit_pairs_only(gpu, oracle, monkeypatch, st, small):
    tile = TILES[st]
    monkeypatch.setenv("ADSB_SMALL_PATH", small)

    def make():
        plants, _ = S.df17_plants(oracle, tile)
        return tile + S.WINDOW, plants

    iq, want, counts = _case(oracle, st, "df17", make)
    plants, n_pass = S.df17_plants(oracle, tile)
    g = S.gate(iq[:, 0])
    for (off, _), (name, _, ok) in zip(plants, S.DF17_VARIANTS * 2):
        assert bool(g[off]) == ok, (name, off)
    assert counts == [n_pass] and len(want) == n_pass - 2  # (the all-tied window survives twice and is no frame)
    with A.AdsbDemod(sample_type=st, max_samples=tile + S.WINDOW, max_out=1 << 12) as d:
        frames, flags = d.demod(iq)
        assert flags == 0
        _eq(frames, want)


@pytest.mark.parametrize("small", ["1", "0"])
@pytest.mark.parametrize("st", STS)
def test_three_channels_with_a_ragged_last_tile_each(gpu, oracle, monkeypatch, st, small):
    import torch
    monkeypatch.setenv("ADSB_SMALL_PATH", small)
    tile, nch = TILES[st], 3
    n, stride = tile + S.WINDOW + 300, tile + S.WINDOW + 304  # (a stride is a multiple of 8 samples)
    host = np.full((nch, stride, 2), 77, dtype=DTYPES[st])  # padding between channels must never be looked at
    wants = []
    for c, k in enumerate((8, 9, 40)):
        def make():
            # the ragged tile: a frame at the last offset the reference looks at (channels 0, 2) or one past it (channel 1)
            return n, S.tile_with(oracle, 0, k, k) + [(n - S.WINDOW - 1 + (c & 1), S.ppm(S.frame_bytes(oracle, 30 + c)))]
        iq, want, counts = _case(oracle, st, ("chan", c), make)
        assert counts == [k, 1 - (c & 1)], (c, counts)
        host[c, :n] = iq
        wants.append(want)
    with A.AdsbDemod(sample_type=st, max_samples=n, max_out=1 << 12, max_channels=nch, host_staging=False) as d:
        t = torch.from_numpy(host).cuda()
        d.demod_device_async(t.data_ptr(), n, nch, stride)
        frames, got_counts, total, flags = d.fetch(n_channels=nch)
        assert flags == 0 and total == len(frames) == sum(len(w) for w in wants)
        pos = 0
        for c in range(nch):
            assert got_counts[c] == len(wants[c])
            _eq(frames[pos:pos + len(wants[c])], wants[c])
            pos += len(wants[c])
