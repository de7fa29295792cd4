"""The builders of tests/cs16_cases.py, checked against the CPU oracle alone: every representative has the root it stands for,
every planted window has the verdict it was built for (from the model of the reference gate AND from the oracle's frame list),
and every tile holds what selects the gate it is meant to exercise."""
import math

import numpy as np
import pytest

from tests import cs16_cases as C
from tests import survivor_cases as S

KINDS = ("f16", "integer", "gate choice", "slicer", "channels")


@pytest.fixture(scope="module")
def built(oracle):
    return C.built(oracle)


def _all(built):
    return [b for key in KINDS for b in built[key]]


def test_representatives_are_the_ends_of_their_class(oracle):
    nsq = lambda iq: iq[0] * iq[0] + iq[1] * iq[1]
    assert nsq(C.rep(1023, "max")) == 933 ** 2 + 422 ** 2 and nsq(C.rep(1023, "min")) == 1023 ** 2
    assert nsq(C.rep(31743, "max")) == 21387 ** 2 + 23458 ** 2 == 31744 ** 2 - 3
    assert sorted(map(abs, C.rep(46339, "min"))) == [32767, 32767]
    assert sorted(map(abs, C.rep(46339, "max"))) == [32766, 32768] and min(C.rep(46339, "max")) == -32768
    assert sorted(map(abs, C.rep(46340, "min"))) == [32767, 32768] and C.rep(46340, "max") == (-32768, -32768)
    assert len(set(C.R)) == len(C.R) == 54 and C.single(0) and not any(C.single(r) for r in C.R[1:])
    pairs, want = [], []
    for r in sorted(set(C.R) | {r + 1 for r in C.R if r < C.TOP} | set(C.SLICER_ROOTS) | {32000, 40000}):
        for which in ("min", "max"):
            for seed in range(4):
                i, q = C.rep(r, which, seed)
                assert -32768 <= i <= 32767 and -32768 <= q <= 32767 and math.isqrt(i * i + q * q) == r
                pairs.append((i, q))
                want.append(r)
        lo, hi = C.class_ends(r)
        assert r * r <= lo[0] <= hi[0] < (r + 1) ** 2
        if r <= 32767:
            assert lo[0] == r * r  # (r, 0)
    pairs += list(C.CORNERS)
    want += [46339, 46339, 46340, 46340]
    assert (oracle.get_magnitude(np.array(pairs, dtype=np.int16)) == np.array(want)).all()


def test_class_ends_against_brute_force():
    """every pair of a few small classes, and of the corner of the range, by enumeration"""
    for m in (0, 1, 2, 3, 7, 180, 181, 182, 255):
        ns = {a * a + b * b for a in range(m + 2) for b in range(m + 2) if math.isqrt(a * a + b * b) == m}
        assert (C.class_ends(m)[0][0], C.class_ends(m)[1][0]) == (min(ns), max(ns)), m
    top = {}
    for a in range(32700, 32769):
        for b in range(32700, 32769):
            top.setdefault(math.isqrt(a * a + b * b), set()).add(a * a + b * b)
    for m in (46338, 46339, 46340):
        assert C.class_ends(m)[1][0] == max(top[m]), m
    assert C.class_ends(46339)[0][0] == min(top[46339]) and C.class_ends(46340)[0][0] == min(top[46340])
    assert len(top[46339]) == 2 and len(top[46340]) == 2 and 46341 not in top


def test_skips_stay_within_the_cap(built):
    assert built["pairs"] == 216 and len(built["skipped"]) <= 8, built["skipped"]
    assert set(built["skipped"]) == {(0, "tie"), (0, "tie, swapped"), (46340, "one class below"), (46340, "one class above")}
    n_windows = sum(len({id(w) for _, w in b.plants}) for key in ("f16", "integer") for b in built[key])
    assert n_windows == 2 * (216 - 4) - 1  # both places, but for the DF17 place of a decisive high of 0


def test_every_buffer_is_what_the_oracle_sees(built, oracle):
    for b in _all(built):
        assert b.n <= 262144 and b.tiles() <= 32, b.name
        assert (oracle.get_magnitude(b.iq) == b.mag).all(), b.name
        g = S.gate(b.mag)
        for off, w in b.plants:
            assert off < b.n - S.WINDOW and bool(g[off]) == w.ok, (b.name, w.name, off)
        rc, got, found = oracle.process_buffer(b.iq)
        want = b.expected()
        assert rc == 0 and found == len(got) == len(want), (b.name, found, len(want))
        assert (got == want).all(), b.name
    assert sum(w.ok for key in ("f16", "integer") for b in built[key] for _, w in b.plants) > 2000
    assert sum(not w.ok for key in ("f16", "integer") for b in built[key] for _, w in b.plants) > 700


def test_decision_windows_cover_every_load_position_and_both_runs(built):
    for key in ("f16", "integer"):
        seen = {}
        for b in built[key]:
            for off, w in b.plants:
                seen.setdefault(id(w), set()).add((off % 4, (off % C.TILE) >= C.TILE // 2))
        assert all(s == {(r, h) for r in range(4) for h in (False, True)} for s in seen.values())


def test_tiles_select_the_gate_they_are_built_for(built):
    for b in built["f16"] + built["slicer"][:1]:
        assert all(b.tile_max(t) < C.F16_LIMIT for t in range(b.tiles())), b.name
    for b in built["integer"] + built["slicer"][1:]:
        assert b.planted_tiles() == list(range(b.tiles())), b.name
        assert all(b.tile_max(t, halo=False) >= C.F16_LIMIT for t in range(b.tiles())), b.name
    for b in built["channels"]:
        assert sorted(b.notes) == list(range(b.tiles())) == [0, 1, 2, 3], b.name
        for t, kind in b.notes.items():
            if kind == "f":
                assert b.tile_max(t) < C.F16_LIMIT, (b.name, t)
            else:
                assert b.tile_max(t, halo=False) >= C.F16_LIMIT, (b.name, t)
        assert b.plants[-1][0] == b.n - S.WINDOW - 1 and b.plants[-1][1].ok
    assert [tuple(b.notes.values()) for b in built["channels"]] == [tuple("ffff"), tuple("iiii"), tuple("fifi")]


def test_gate_choice_tiles_hold_one_big_sample_where_it_is_meant_to_be(built):
    names = []
    for b in built["gate choice"]:
        counts = S.survivors_per_tile(b.mag, C.TILE)
        for t, (name, p) in b.notes.items():
            own = t % 2 == 0  # the tile under test; odd tiles are the next tile of a halo placement
            big = np.nonzero(b.mag[t * C.TILE:(t + 1) * C.TILE + (C.HALO if own else 0)] >= C.F16_LIMIT)[0]
            assert list(big) == [p], (b.name, name, list(big))
            if own:
                names.append(name)
                # the reference's survivors of the tile: none, but for the window that no big sample decides
                assert counts[t] == (1 if name.startswith("last sample") else 0), (b.name, name, counts[t])
                for wave in range(4):
                    if name.endswith(f"wave {wave}"):
                        assert p < C.TILE and C.wave_of(p) == wave
                if p >= C.TILE:
                    assert C.wave_of(p) == 0 and t + 1 in b.notes
            else:
                assert counts[t] == 1  # what the next tile makes of it: an early sample of its own, and its control frame
        assert all(counts[t] == 1 for t in range(1, len(counts), 2)), b.name
    kinds = ("negative low -0", "negative low 40000", "negative low corner", "NaN high (preamble)", "NaN high (DF17)")
    for where in ("wave 0", "wave 1", "wave 2", "wave 3", "sample 8191", "halo 0"):
        for kind in kinds:
            assert any(n.startswith(kind) and n.endswith(where) for n in names), (kind, where)
    assert any(n.startswith("NaN high (preamble) at 0") and n.endswith("sample 0") for n in names)
    assert sum(n.startswith("last sample") and n.endswith("halo 238") for n in names) == 2


def test_slicer_frames_tie_where_the_frame_has_a_zero(built, oracle):
    seen = set()
    for b in built["slicer"]:
        for off, w in b.plants:
            bits = np.unpackbits(np.frombuffer(w.frame, dtype=np.uint8))
            first, second = w.mags[16::2], w.mags[17::2]
            n = (w.iq.astype(np.int64) ** 2).sum(axis=1)
            assert (first[bits == 1] == second[bits == 1] + 1).all()
            if "ties" in w.name:
                assert (first[bits == 0] == second[bits == 0]).all()
                assert (n[16::2][bits == 0] > n[17::2][bits == 0]).all()  # a slicer on I^2 + Q^2 slices these as 1
            else:
                assert (first[bits == 0] + 1 == second[bits == 0]).all()
            seen.add((w.name, off % 2))
    assert seen == {(f"slicer {k} at {m}", a) for k in ("ties", "steps") for m in C.SLICER_ROOTS for a in (0, 1)}
