"""The conditions the position sweeps rest on (tests/sweep_cases.py; CPU tier, the device tests are tests/test_gpu_position_sweep.py
and tests/ab_cases.py::test_position_sweep).

For every buffer the device tests use: the oracle's list IS the planted list (nothing missing, nothing else, every field), the
planted offsets mod the tile length are 0 .. tile - 1 each once, every data bit 5..87 is repaired somewhere, every level meets
every class, the model gate passes at every planted offset, and the samples are real (I, Q) pairs whose roots are the modelled
magnitudes.  And the reason the sweeps exist: exchanging two neighbouring samples at one in-tile offset of every tile leaves the
constant buffer's list as it was and changes a sweep's."""
import math

import numpy as np
import pytest

from tests import crc_cases as C
from tests import survivor_cases as S
from tests import sweep_cases as W


@pytest.mark.parametrize("name", list(W.CASES))
def test_the_oracles_list_is_the_plan(oracle, name):
    s, want, seconds = W.reference(oracle, name)
    dtype, tile, stride, levels, rotate, shift, big = W.CASES[name]
    assert s.iq.dtype == dtype and s.tile == tile and len(s.planted) == tile
    W.compare(want, s.planted, tile, name)                                    # zero missing, zero wrong, zero extra
    off = s.planted["offset"].astype(np.int64)
    assert (np.diff(off) == stride).all() and 0 < off[0] <= W.LEAD + tile and off[0] % tile == (W.LEAD - shift) % tile
    assert (np.sort(off % tile) == np.arange(tile)).all()                      # every in-tile offset, once
    assert len(s.iq) == off[-1] + W.WINDOW + W.TAIL                            # 240 samples and a ragged tail behind the last frame
    assert len({r.tobytes() for r in s.planted["bytes"]}) == tile              # distinct frames
    assert (s.planted["bytes"][:, 0] == 0x8D).all() and all(C.syndrome(r) == 0 for r in s.planted["bytes"][::97])
    # classes, bits and levels
    flipped = s.class_of == W.FLIP
    assert (s.planted["status"] == flipped).all() and (s.planted["fixed_bit"][~flipped] == 0xFF).all()
    assert set(s.planted["fixed_bit"][flipped].tolist()) == set(W.FLIP_BITS)
    assert all(W.tie_ok(oracle, dtype, lv) for lv in levels)                   # no level had to give up its TIE frames
    pairs = set(zip(s.level_of.tolist(), s.class_of.tolist()))
    assert pairs == {(lv, c) for lv in range(len(levels)) for c in (W.CLEAN, W.FLIP, W.TIE)}
    for lv, (hi, lo, bg) in enumerate(levels):                                 # the frames are there at their levels
        k = int(np.nonzero((s.level_of == lv) & (s.class_of == W.CLEAN))[0][0])
        w = s.mag[off[k]:off[k] + W.WINDOW]
        assert w.max() == hi and w.min() == lo and (w[list(S.PRE_HIGHS)] == hi).all()
    # the gate of the model
    g = W.gate(s.mag)
    assert g[off].all()
    per_tile = W.survivors_per_tile(s.mag, tile)
    assert (g[:50_000 - W.WINDOW] == S.gate(s.mag[:50_000])).all()               # (the 32-bit gate is survivor_cases' gate)
    # the samples
    iq = s.iq.astype(np.int64)
    n = iq[:, 0] * iq[:, 0] + iq[:, 1] * iq[:, 1]
    m = s.mag.astype(np.int64)
    assert ((n >= m * m) & (n < (m + 1) * (m + 1))).all()
    assert (oracle.get_magnitude(s.iq[:200_000].astype(np.int16)) == s.mag[:200_000]).all()
    assert all(math.isqrt(int(v)) == int(r) for v, r in zip(n[:5000], m[:5000]))
    some = m > 0
    assert (iq[some] != 0).all()                                               # both components, wherever the root allows
    assert all((iq[some, c] > 0).any() and (iq[some, c] < 0).any() for c in (0, 1))
    assert (np.diff(s.mag) != 0).sum() > len(s.mag) // 2 and _longest_run(s.mag) < 100
    # the big samples
    top = max(hi for hi, lo, bg in levels)
    if big:
        assert top >= W.F16_LIMIT and len(s.big_at) == len(per_tile)
        for t, p in enumerate(s.big_at):
            assert t * tile <= p < (t + 1) * tile and s.mag[p] >= W.F16_LIMIT
            assert not ((off <= p) & (p < off + W.WINDOW)).any()               # outside every planted window
    else:
        assert s.mag.max() == top and (top < W.F16_LIMIT or dtype == np.int8) and not s.big_at
    print(f"\n{name}: {len(s.iq)} samples, {len(want)} frames, survivors per tile {per_tile.min()} .. {per_tile.max()} "
          f"({len(per_tile)} tiles), oracle {seconds:.2f} s")


def _longest_run(mag):
    edges = np.nonzero(np.diff(mag) != 0)[0]
    return int(np.diff(np.r_[-1, edges, len(mag) - 1]).max())


def test_shifts_move_every_frame_to_another_offset(oracle):
    base = W.built(oracle, "i8 dense").planted["offset"].astype(np.int64)
    tile = 16384
    for name, shift in (("i8 dense shift 1", 1), ("i8 dense shift tile/2+5", tile // 2 + 5)):
        off = W.built(oracle, name).planted["offset"].astype(np.int64)
        assert ((off - base) % tile == -shift % tile).all()
    assert ((W.built(oracle, "i8 dense shift 1").planted["offset"] ^ base.astype(np.uint64)) & 1).all()  # the other half of a dword


def test_representatives():
    """i8: every pair with both components non-zero, and the others of a root that has none; CS16: drawn pairs, each checked with
    math.isqrt when it was drawn"""
    seen = 0
    for m in range(182):
        tab = W.reps(np.int8, m).astype(np.int64)
        assert len(np.unique(tab, axis=0)) == len(tab)
        assert all(math.isqrt(int(a * a + b * b)) == m for a, b in tab)
        seen += len(tab)
    assert seen == 255 * 255 + 1                                               # 65 025 pairs without a zero, and (0, 0)
    assert W.reps(np.int8, 181).tolist() == [[-128, -128]]
    for m in sorted({v for lv in W.LEVELS_CS16_BIG for v in lv} | {0, W.BIG_ROOT}):
        tab = W.reps(np.int16, m).astype(np.int64)
        assert all(math.isqrt(int(a * a + b * b)) == m for a, b in tab)
        if m > 1:
            assert (tab < 0).any(axis=0).all() and (tab > 0).any(axis=0).all()
        if m > 100:
            assert len(np.unique(tab, axis=0)) > len(tab) // 2
            n = tab[:, 0] ** 2 + tab[:, 1] ** 2                                # the whole class [m^2, (m + 1)^2), not its first value
            assert n.min() < m * m + m // 2 and n.max() > m * m + m + m // 2


def test_what_the_gaps_give_a_window_inside_a_tie_frame_is_no_frame():
    """sweep_cases.build: behind zeros, a run of ones to the window's end, or seven or eight ones and zeros again, is neither a
    codeword nor one repaired bit from one"""
    frames = {0} | set(C.DATA_SYN)
    assert all(C._polymod((1 << b) - 1) not in frames for b in range(1, 113))
    assert all(C._polymod(((1 << w) - 1) << c) not in frames for w in (7, 8) for c in range(113 - w))


def test_the_constant_buffer_is_blind_to_an_exchange_and_a_sweep_is_not(oracle):
    residue = 1000
    const = np.full((40_000, 2), 5, dtype=np.int8)
    rc, want, found = oracle.process_buffer(const)
    rc2, got, found2 = oracle.process_buffer(W.swap_at(const, 16384, residue))
    assert rc == rc2 == 0 and found == found2 == 40_000 - W.WINDOW and (got == want).all()
    s, want, _ = W.reference(oracle, "cs16 dense")
    swapped = W.swap_at(s.iq, s.tile, residue)
    assert (swapped != s.iq).any(axis=1).sum() > len(s.iq) // s.tile             # (two samples per tile, where they differ)
    assert (np.sort(swapped.view(np.uint32).ravel()) == np.sort(s.iq.view(np.uint32).ravel())).all()  # a permutation
    rc, got, found = oracle.process_buffer(swapped, max_out=4 * s.tile)
    text = W.differences(got, want, s.tile)
    assert rc == 0 and text is not None
    # the frames that changed are those over the exchanged samples, and the report says where
    now = {int(r["offset"]): r.tobytes() for r in got}
    changed = [int(r["offset"]) for r in want if now.get(int(r["offset"])) != r.tobytes()]
    assert len(changed) > 100 and all((residue + 1 - o % s.tile) % s.tile <= W.WINDOW for o in changed)
    assert "in-tile offsets missing: " in text and "tiles concerned: " in text


def test_the_report_names_tiles_offsets_and_ranges(oracle):
    s = W.built(oracle, "cs16 dense")
    want = s.planted
    assert W.differences(want.copy(), want, s.tile) is None
    got = want.copy()
    by_offset = np.argsort(got["offset"] % s.tile)                            # the frames at in-tile offsets 64 .. 127: one lane's run
    got["bytes"][by_offset[64:128], 3] ^= 1
    got = np.delete(got, by_offset[[5, 6, 7, 4000]])
    text = W.differences(got, want, s.tile)
    assert "4 missing, 64 wrong, 0 extra" in text
    assert "in-tile offsets missing: 5-7, 4000" in text and "in-tile offsets wrong: 64-127" in text
    k = int(by_offset[5])
    assert f"missing  tile {int(want['offset'][k]) // s.tile} + 5: {want['bytes'][k].tobytes().hex()}" in text
    with pytest.raises(AssertionError, match="in-tile offsets wrong: 64-127"):
        W.compare(got, want, s.tile, "a mutant")
    assert W.ranges([]) == "none" and W.ranges([3, 1, 2, 9]) == "1-3, 9"


def test_slices_keep_the_in_tile_offsets(oracle):
    for name in ("cs16 dense", "i8 sparse"):
        s = W.built(oracle, name)
        cut = W.slices(len(s.iq), s.tile)
        assert all(a % (W.SLICE_TILES * s.tile) == 0 and W.WINDOW < n <= W.SLICE_TILES * s.tile + W.WINDOW for a, n in cut)
        assert all(n == W.SLICE_TILES * s.tile + W.WINDOW for a, n in cut[:-1]) and cut[-1][0] + cut[-1][1] == len(s.iq)
        assert sum(n - W.WINDOW for a, n in cut) == len(s.iq) - W.WINDOW       # every offset in one slice
    s, want, _ = W.reference(oracle, "cs16 dense")
    parts, (a, padded, padded_want) = W.slice_reference(oracle, "cs16 dense")
    joined = np.concatenate([w for _, _, w in parts])
    joined["offset"] += np.repeat([a for a, _, _ in parts], [len(w) for _, _, w in parts]).astype(np.uint64)
    W.compare(joined, want, s.tile, "the slices' lists, joined")
    last = parts[-1][2]
    assert len(padded) == W.SLICE_TILES * s.tile + W.WINDOW and (padded_want[:len(last)] == last).all()
    assert (padded_want["offset"][len(last):] >= len(parts[-1][1]) - W.WINDOW).all()
