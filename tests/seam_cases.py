"""Buffers with a frame at every offset around every seam of a time-sharded buffer (adsb_group_*, sharding.plan), and
what the oracle makes of the whole buffer.  Shared by tests/test_seam_cases.py (CPU: the cases can show a failure) and
tests/test_gpu_seams.py.

A constant buffer passes the gate at every offset (ties pass), slices to 112 zero bits and has CRC 0: one all-zero
frame per offset.  So the background is the synthetic stream without frames (frame_pct 0: noise only), and around
every seam s the samples [s - 300, s + 540) are the constant (3, 4): every offset of [s - 300, s + 300] has its whole
240-sample window inside the constant stretch.  A member that examines one offset too few or too many, a halo one
sample short, a lost or a doubled list entry at a seam changes the list."""
import numpy as np

import air_rs_amd as A
from air_rs_amd import sharding

WORLDS = (2, 3, 8)
RAGGED = (0, 1, 7, 8, 9)          # total = world * 4096 + 240 + r: even and ragged last members
BEFORE, AFTER, SURE = 300, 540, 30
CONSTANT = (3, 4)
FEW = (8, 9, 16, 20)              # 240 + k samples over 8 members: fewer offsets than members
TYPES = {"i8": A.ADSB_SAMPLE_I8, "i16": A.ADSB_SAMPLE_I16}


def total_of(world, r):
    return world * 4096 + A.WINDOW + r


def seams_of(total, world):
    """First offsets of the members after the first that own something."""
    return [first for first, ns, noff in A.group_plan(total, world)[1:] if noff]


_cache = {}


def seam_buffer(oracle, st, total, world):
    """(iq, want, seams): the buffer, the oracle's list over the whole of it, the seams of the plan for (total, world)."""
    key = (st, total, world)
    if key not in _cache:
        iq = A.synth_fill_host(A.synth_default(seed=0x5EA3 + world, frame_pct=0), st, 0, 0, total)
        seams = seams_of(total, world)
        for s in seams:
            iq[max(s - BEFORE, 0):min(s + AFTER, total)] = CONSTANT
        rc, want, found = oracle.process_buffer(iq, max_out=total)
        assert rc == 0 and found == len(want)
        iq.setflags(write=False)
        want.setflags(write=False)
        _cache[key] = (iq, want, seams)
    return _cache[key]


def few_offsets_buffer(st, k):
    return np.full((A.WINDOW + k, 2), CONSTANT, dtype=np.int8 if st == A.ADSB_SAMPLE_I8 else np.int16)


def python_shards(total, world):
    return [(sh.first_sample, sh.n_samples, sh.n_offsets) for sh in sharding.plan(total, world)]
