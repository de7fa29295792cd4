"""Launches of many one-tile channels for finish_order's exchange (finish_block, adsb_kernels.hip), and a model of it.

A tile costs one finishing slot whether it holds 16 384 offsets or 8, so a launch of many short channels, one tile each,
reaches any workgroup count with a few tens of MB of samples.  The channels are dealt from a small pool of distinct
one-tile buffers; the CPU oracle runs once per pool entry, and the launch's whole list is the concatenation of the
entries' lists in channel order -- every frame's place depends on the totals of all workgroups before its own.

Every shape comes from adsb_debug_finish_geometry: T tiles per workgroup, F workgroups per second-level sum, L the largest
grid that exchanges in one level, S second-level sums read per round.

Pool entries are cut from synth_fill_host streams (slot_len 256, every second slot a frame, differing seeds) around the
planted frames, so they hold 0, 1 or 2 frames.  A buffer of 256 offsets cannot hold three whole frames side by side:
the entries with three and more carry a run of 239 + k constant samples at their front, which decodes to one all-zero
frame at each of the first k offsets (tests/test_gpu_handover_edges.py), k up to 31 -- beyond 16 the tile is finished by
a whole wave (finish_big_tile), still inside its own slots."""
import collections
import ctypes as C
import itertools

import numpy as np

import air_rs_amd as A
from air_rs_amd import _lib

KQUOTA = 32                    # a tile's own slots (kQuota, adsb_kernels.h; "its own 32 slots", include/adsb_hip.h)
WINDOW = A.WINDOW
SLOT = 256                     # the synthetic stream's shortest slot: one frame per 256 samples at the most
POOL = 96                      # entries per pool
SAMPLES, SAMPLES_BIG = 496, 248  # per channel: 256 offsets, 8 offsets; one tile of either sample type
CONSTANT = (3, 4)
RUNS = (3, 4, 5, 6, 7, 8, 11, 16, 17, 24, 31)
DTYPES = {A.ADSB_SAMPLE_I8: np.int8, A.ADSB_SAMPLE_I16: np.int16}
DEAL_SEED = 20240229

Geometry = collections.namedtuple("Geometry", "T F L S")
Pool = collections.namedtuple("Pool", "iq lists counts frames starts")
Pool.__doc__ = """iq: (K, n_samples, 2) samples; lists: the oracle's list per entry; counts: their lengths; frames: the lists
laid end to end; starts: where each entry's list begins in `frames`."""
Case = collections.namedtuple("Case", "pool perm counts prefix frames")
Case.__doc__ = """One launch: channel c holds pool entry perm[c]; counts: expected frames per channel; prefix: frames
before each channel (and the total); frames: the expected list."""


def geometry():
    v = [C.c_uint32() for _ in range(4)]
    assert _lib.load().adsb_debug_finish_geometry(*[C.byref(x) for x in v]) == A.ADSB_OK
    return Geometry(*[x.value for x in v])


def shapes(g):
    """name -> (workgroups, tiles of the last workgroup, samples per channel)"""
    return {"flat": (g.L, g.T, SAMPLES),                   # the last flat size
            "first": (g.L + 1, 1, SAMPLES),                # first two-level size; a last group of one workgroup, one tile
            "whole": (g.L + g.F, g.T, SAMPLES),            # the launch's last workgroup is its group's publisher
            "ragged": (g.L + g.F + 1, 7, SAMPLES),         # a one-workgroup group behind a whole one; ragged last workgroup
            "big": (g.S * g.F + g.F + 1, 1, SAMPLES_BIG)}  # S + 1 earlier groups for the last workgroup: a second round


def tiles_of(g, workgroups, last):
    return (workgroups - 1) * g.T + last


# ---- the pool ---------------------------------------------------------------------------------------------------------
def _cuts(st, n_samples):
    """Buffers of n_samples cut around the frames the synthetic stream plants: the frame starts up to 4 samples before
    the buffer (then it is not in it) to 4 offsets past the last one."""
    n_off = n_samples - WINDOW
    for seed in itertools.count(7001):
        cfg = A.synth_default(seed=seed, slot_len=SLOT, frame_pct=50)
        stream = A.synth_fill_host(cfg, st, 0, 0, 1 << 16)
        for slot in range(1, (1 << 16) // SLOT - 4):
            has, start, *_ = A.synth_slot(cfg, 0, slot)
            at = int(start) + 4 - (slot * 37 + seed * 11) % (n_off + 8)
            if has and 0 <= at and at + n_samples <= len(stream):
                yield stream[at:at + n_samples].copy()


_POOLS = {}


def pool(oracle, st, n_samples, size=POOL):
    """`size` distinct buffers of n_samples samples holding 0, 1, (2,) and 3 .. KQUOTA frames in turn; built once per
    (sample type, length), shared, read-only."""
    key = (st, n_samples, size)
    if key in _POOLS:
        return _POOLS[key]
    n_off = n_samples - WINDOW
    kinds = [0, 1, 2, "run"] if n_off >= SLOT else [0, 1, "run"]   # (two planted frames lie a slot apart)
    runs = [k for k in RUNS if k <= n_off]
    cuts, seen, iq, lists = _cuts(st, n_samples), set(), [], []
    for i in range(size):
        kind = kinds[i % len(kinds)]
        for tries in itertools.count():
            assert tries < 20000, (key, i, kind)
            buf = next(cuts)
            if kind == "run":
                buf[:WINDOW - 1 + runs[(i // len(kinds)) % len(runs)]] = CONSTANT
            rc, want, found = oracle.process_buffer(buf, max_out=n_off + 1)
            ok = (3 <= found <= KQUOTA) if kind == "run" else found == kind
            if rc == 0 and ok and found == len(want) and buf.tobytes() not in seen:
                break
        seen.add(buf.tobytes())
        iq.append(buf)
        lists.append(want.astype(A.FRAME_DTYPE))
    _POOLS[key] = _pool_of(np.stack(iq), lists)
    return _POOLS[key]


def _pool_of(iq, lists):
    counts = np.array([len(x) for x in lists], dtype=np.int64)
    frames = np.concatenate(lists)
    starts = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.int64)
    for arr in (iq, counts, frames, starts):
        arr.setflags(write=False)
    return Pool(iq, lists, counts, frames, starts)


def with_constant(oracle, p):
    """p and one more entry, of constant samples: one frame per offset, far over a tile's own slots."""
    buf = np.empty(p.iq.shape[1:], dtype=p.iq.dtype)
    buf[:] = CONSTANT
    rc, want, found = oracle.process_buffer(buf, max_out=len(buf))
    assert rc == 0 and found == len(want)
    return _pool_of(np.concatenate([p.iq, buf[None]]), list(p.lists) + [want.astype(A.FRAME_DTYPE)])


# ---- dealing ----------------------------------------------------------------------------------------------------------
def deal(p, tiles, g, seed=DEAL_SEED):
    """Channel c takes entry perm[c]: a fixed-seed draw with no period.  The last channel takes an entry with two frames
    or more, so that a last workgroup of one tile still has frames to put in the wrong place.  Where two adjacent groups
    of F workgroups happen to hold equally many frames, the later one's first channel takes the pool's next entry
    (another count: neighbours in the pool are of different kinds) -- equal sums would hide a sum read from the wrong
    group."""
    perm = np.random.default_rng(seed).integers(0, len(p.counts), tiles)
    perm[-1] = int(np.nonzero(p.counts >= 2)[0][0])
    while True:
        sums = group_sums(workgroup_totals(p.counts[perm], g), g)
        same = np.nonzero(sums[1:] == sums[:-1])[0] + 1
        if len(same) == 0:
            return perm
        first = same[:1] * g.F * g.T                     # one at a time: the change moves this pair and the next
        perm[first] = (perm[first] + 1) % len(p.counts)


def case_of(p, perm):
    counts = p.counts[perm]
    prefix = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    inside = np.arange(prefix[-1]) - np.repeat(prefix[:-1], counts)
    frames = p.frames[np.repeat(p.starts[perm], counts) + inside]
    for arr in (perm, counts, prefix, frames):
        arr.setflags(write=False)
    return Case(p, perm, counts, prefix, frames)


_CASES = {}


def case(oracle, st, name):
    """The launch of shape `name` (shapes()), dealt from the pool of its length; built once, shared, read-only."""
    key = (st, name)
    if key not in _CASES:
        g = geometry()
        workgroups, last, n_samples = shapes(g)[name]
        p = pool(oracle, st, n_samples)
        _CASES[key] = case_of(p, deal(p, tiles_of(g, workgroups, last), g))
    return _CASES[key]


def clipped_counts(c, cap):
    """per-channel counts of the first `cap` frames of the list (adsb_fetch)"""
    return np.minimum(c.prefix[1:], cap) - np.minimum(c.prefix[:-1], cap)


# ---- the model ----------------------------------------------------------------------------------------------------------
def workgroup_totals(counts, g):
    pad = (-len(counts)) % g.T
    return np.concatenate([counts, np.zeros(pad, dtype=counts.dtype)]).reshape(-1, g.T).sum(axis=1)


def group_sums(totals, g):
    """what the last workgroup of every whole group of F publishes"""
    whole = len(totals) // g.F
    return totals[:whole * g.F].reshape(whole, g.F).sum(axis=1)


def before_model(totals, g, wrong=None):
    """`before` of every workgroup as finish_block adds it up from the workgroups' totals; wrong: a MUTANTS name."""
    n = len(totals)
    w = np.arange(n)
    cum = np.concatenate([[0], np.cumsum(totals)])
    if n <= g.L:                                          # one level: every word before this one
        before = cum[:-1].copy()
        if wrong == "flat: the word just before missing":
            before[1:] -= totals[:-1]
        elif wrong == "flat: word 0 missing":
            before[1:] -= totals[0]
        else:
            assert wrong is None, wrong
        return before
    grp, r = w // g.F, w % g.F
    in_grp = cum[w] - cum[grp * g.F]                      # the words of its own group, lane < r
    sums = group_sums(totals, g).copy()
    if wrong == "two-level: the publisher's own total missing from its sum":
        sums -= totals[g.F - 1::g.F][:len(sums)]
    csum = np.concatenate([[0], np.cumsum(sums)])
    earlier = csum[grp]                                   # the sums of the earlier groups, k < grp
    if wrong == "two-level: the in-group word just before missing":
        in_grp = in_grp - np.where(r >= 1, totals[np.maximum(w - 1, 0)], 0)
    elif wrong == "two-level: the in-group word of lane 0 missing":
        in_grp = in_grp - np.where(r >= 1, totals[grp * g.F], 0)
    elif wrong == "two-level: the in-group words missing":
        in_grp = np.zeros_like(in_grp)
    elif wrong == "two-level: the last earlier sum missing":
        earlier = csum[np.maximum(grp - 1, 0)]
    elif wrong == "two-level: the earlier sums missing":
        earlier = np.zeros_like(earlier)
    elif wrong == "two-level: the sums beyond the first round missing":
        earlier = csum[np.minimum(grp, g.S)]
    else:
        assert wrong in (None, "two-level: the publisher's own total missing from its sum"), wrong
    return in_grp + earlier


# (name, does a launch of this many workgroups run the code it breaks)
MUTANTS = (("flat: the word just before missing", lambda n, g: n <= g.L),
           ("flat: word 0 missing", lambda n, g: n <= g.L),
           ("two-level: the in-group word just before missing", lambda n, g: n > g.L),
           ("two-level: the in-group word of lane 0 missing", lambda n, g: n > g.L),
           ("two-level: the in-group words missing", lambda n, g: n > g.L),
           ("two-level: the last earlier sum missing", lambda n, g: n > g.L),
           ("two-level: the earlier sums missing", lambda n, g: n > g.L),
           ("two-level: the publisher's own total missing from its sum", lambda n, g: n > g.L),
           ("two-level: the sums beyond the first round missing", lambda n, g: n > g.L and (n - 1) // g.F > g.S))


def model_list(c, g, wrong=None, descending=False):
    """The list finish_order writes with the workgroups' starts of before_model: every tile's frames at its workgroup's
    start plus the frames of the workgroup's earlier tiles; places nobody writes stay zero.  Two tiles may claim one
    place when a start is wrong, and the kernel does not say who writes last: ascending tile order or descending."""
    totals = workgroup_totals(c.counts, g)
    before = before_model(totals, g, wrong)
    tile = np.arange(len(c.counts))
    first_of_wg = c.prefix[:-1][(tile // g.T) * g.T]
    pos = before[tile // g.T] + (c.prefix[:-1] - first_of_wg)
    dst = np.repeat(pos, c.counts) + (np.arange(c.prefix[-1]) - np.repeat(c.prefix[:-1], c.counts))
    src = np.arange(c.prefix[-1])
    keep = (dst >= 0) & (dst < c.prefix[-1])
    dst, src = dst[keep], src[keep]
    if descending:
        dst, src = dst[::-1], src[::-1]
    out = np.zeros(c.prefix[-1], dtype=A.FRAME_DTYPE)
    order = np.argsort(dst, kind="stable")               # of the writes to one place, the last one stays
    dst, src = dst[order], src[order]
    last = np.concatenate([dst[1:] != dst[:-1], [True]])
    out[dst[last]] = c.frames[src[last]]
    return out
