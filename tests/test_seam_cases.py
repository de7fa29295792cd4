"""The seam cases of tests/seam_cases.py can show a failure (CPU tier): both plans make the same cut, on 8-sample
boundaries, tiling every offset once; and the oracle's list holds a frame at every offset around every seam."""
import numpy as np
import pytest

import air_rs_amd as A
from tests import seam_cases as S


@pytest.mark.parametrize("world", S.WORLDS)
def test_both_plans_make_the_same_cut(lib, world):
    for r in S.RAGGED:
        total = S.total_of(world, r)
        native = A.group_plan(total, world)
        assert native == S.python_shards(total, world)
        pos = 0
        for first, ns, noff in native:
            assert first % 8 == 0 or noff == 0
            assert noff > 0 and first == pos and ns == noff + A.WINDOW and first + ns <= total
            pos += noff
        assert pos == total - A.WINDOW
        assert len(S.seams_of(total, world)) == world - 1
    for k in S.FEW:
        native = A.group_plan(A.WINDOW + k, 8)
        assert native == S.python_shards(A.WINDOW + k, 8)
        owned = [noff for first, ns, noff in native]
        assert sum(owned) == k and owned[0] == 8 and all(first % 8 == 0 for first, ns, noff in native if noff)
        assert not any(owned[3:]) and all(ns == 0 for (first, ns, noff) in native if noff == 0)


@pytest.mark.parametrize("t", S.TYPES)
@pytest.mark.parametrize("world", S.WORLDS)
def test_a_frame_at_every_offset_around_every_seam(oracle, world, t):
    for r in S.RAGGED:
        total = S.total_of(world, r)
        iq, want, seams = S.seam_buffer(oracle, S.TYPES[t], total, world)
        off = want["offset"].astype(np.int64)
        assert (np.diff(off) > 0).all() and len(want) < 1 << 14
        have = set(off.tolist())
        for s in seams:
            assert all(o in have for o in range(s - S.SURE, s + S.SURE + 1)), (world, r, s)
            assert all(o in have for o in range(s - S.BEFORE, s + S.BEFORE + 1)), (world, r, s)
        near = np.zeros(total, dtype=bool)
        for s in seams:
            near[max(s - S.BEFORE - A.WINDOW, 0):s + S.AFTER] = True
        assert near[off].all()        # the noise between the stretches carries no frame
        at_seams = want[np.isin(off, seams)]
        assert len(at_seams) == len(seams) and not at_seams["bytes"].any() and not at_seams["status"].any()


@pytest.mark.parametrize("t", S.TYPES)
def test_few_offsets_buffers(oracle, t):
    for k in S.FEW:
        rc, want, found = oracle.process_buffer(S.few_offsets_buffer(S.TYPES[t], k))
        assert rc == 0 and found == k and (want["offset"] == np.arange(k)).all() and not want["bytes"].any()
