"""finish_order's exchange of workgroup totals (finish_block, adsb_kernels.hip) at the grid sizes where it takes another
path, by launches of many one-tile channels (tests/finish_cases.py; tests/test_finish_cases.py shows on the CPU that
these launches cannot hide a wrong `before`).  With T tiles per workgroup, F workgroups per second-level sum, L the
largest one-level grid and S sums per round, all from adsb_debug_finish_geometry:

  flat    L workgroups            the last one-level size
  first   L + 1, last of 1 tile   the first two-level size; the last group is one workgroup holding one tile
  whole   L + F                   the launch's last workgroup publishes its group's sum
  ragged  L + F + 1, last of 7    a one-workgroup group behind a whole one; a ragged last workgroup
  big     S F + F + 1, last of 1  S + 1 earlier groups for the last workgroup: the second round of the sums' loop

Every launch is compared whole: flags, total, the list byte for byte with the concatenation of the oracle's per-entry
lists, the per-channel counts, and a second run on the same context.

Which of these fails if `before` lost a term (tests/test_finish_cases.py, MUTANTS): the in-group words -- every case
but `flat`; the earlier groups' sums -- every case but `flat`; the sums beyond the first S -- `big` alone, in its last
workgroup's two frames and the total; the publisher's own total -- every case but `flat`."""
import time

import numpy as np
import pytest

import air_rs_amd as A
from tests import finish_cases as FC

pytestmark = pytest.mark.gpu
I8, I16 = A.ADSB_SAMPLE_I8, A.ADSB_SAMPLE_I16
GIB = 1 << 30


@pytest.fixture(autouse=True)
def two_kernel_path(monkeypatch):
    monkeypatch.setenv("ADSB_SMALL_PATH", "0")     # (read at adsb_create; none of these tile counts fits one dispatch)


@pytest.fixture(scope="module")
def g(gpu):
    return FC.geometry()


def _device_input(c):
    """The launch's samples, built on the device by indexing the pool: (tiles, n_samples, 2), channel after channel."""
    import torch
    pool = torch.from_numpy(np.array(c.pool.iq)).cuda()          # (copies: the shared arrays are read-only)
    iq = pool[torch.from_numpy(np.array(c.perm)).cuda()].contiguous()
    assert iq.shape == (len(c.perm),) + c.pool.iq.shape[1:] and iq.data_ptr() % 16 == 0
    return iq


def _launch(d, iq):
    d.demod_device_async(iq.data_ptr(), iq.shape[1], n_channels=iq.shape[0], channel_stride=iq.shape[1])
    return d.fetch()


def _same_list(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    if got.tobytes() != want.tobytes():
        bad = np.nonzero(got != want)[0]
        raise AssertionError((what, len(bad), bad[:5], got[bad[:3]], want[bad[:3]]))


def _check(d, iq, c, what):
    """One launch and a second one on the same context against the expected list -> the seconds both took."""
    t0 = time.perf_counter()
    frames, counts, total, flags = _launch(d, iq)
    assert flags == 0, (what, flags)
    assert total == len(frames) == c.prefix[-1], (what, total, len(frames), int(c.prefix[-1]))
    _same_list(frames, c.frames, what)
    assert np.array_equal(np.asarray(counts, dtype=np.int64), c.counts), what
    again, counts2, total2, flags2 = _launch(d, iq)
    assert (flags2, total2) == (0, total) and again.tobytes() == frames.tobytes() and list(counts2) == list(counts), what
    return time.perf_counter() - t0


def _ctx(c, st=I8, max_out=None):
    return A.AdsbDemod(sample_type=st, max_samples=c.pool.iq.shape[1], max_channels=len(c.perm),
                       max_out=int(c.prefix[-1]) + 64 if max_out is None else max_out, host_staging=False)


# ---- 1: the first four shapes, i8, the product's scan ---------------------------------------------------------------------
@pytest.mark.parametrize("name", ["flat", "first", "whole", "ragged"])
def test_shapes(gpu, oracle, g, name):
    c = FC.case(oracle, I8, name)
    iq = _device_input(c)
    with _ctx(c) as d:
        assert d.scan == "root"
        took = _check(d, iq, c, name)
    print(f"{name}: {len(c.perm)} channels, {int(c.prefix[-1])} frames, two launches compared in {took:.2f} s")
    del iq


# ---- 2: CS16 (its own tile length; a channel is still one tile) ----------------------------------------------------------
def test_cs16_first_two_level_size(gpu, oracle, g):
    c = FC.case(oracle, I16, "first")
    iq = _device_input(c)
    with _ctx(c, I16) as d:
        took = _check(d, iq, c, "cs16 first")
    print(f"cs16 first: {len(c.perm)} channels, {int(c.prefix[-1])} frames, two launches compared in {took:.2f} s")
    del iq


# ---- 3: one context: two-level, flat over the older second-level words, two-level again; then across the epoch wrap ------
def test_same_context_in_order(gpu, oracle, g):
    first, flat = FC.case(oracle, I8, "first"), FC.case(oracle, I8, "flat")
    iq_first, iq_flat = _device_input(first), _device_input(flat)
    assert len(first.perm) > len(flat.perm) and first.prefix[-1] != flat.prefix[-1]
    with _ctx(first) as d:
        # every _check is two launches: both result sets take each shape
        for k, (iq, c) in enumerate(((iq_first, first), (iq_flat, flat), (iq_first, first))):
            _check(d, iq, c, ("in order", k))
        # one more launch shifts the result sets against the shapes
        frames, counts, total, flags = _launch(d, iq_flat)
        assert flags == 0 and total == flat.prefix[-1]
        _same_list(frames, flat.frames, "flat, odd")
        _check(d, iq_first, first, "first, shifted")
        # the epoch wraps with second-level words in place: launch 2^30 - 2 has epoch 2^30 - 1, the next one 0 (the
        # words are zeroed before it), the third 1
        d.set_launch_index((1 << 30) - 2)
        for k in range(3):
            frames, counts, total, flags = _launch(d, iq_first)
            assert flags == 0 and total == first.prefix[-1], (k, flags, total)
            _same_list(frames, first.frames, ("wrap", k))
            assert np.array_equal(np.asarray(counts, dtype=np.int64), first.counts), k
    del iq_first, iq_flat


# ---- 4: the big shape: more than S earlier groups ------------------------------------------------------------------------
def _big_bytes(g, c, max_out):
    """What the launch needs on the device: the samples and the index they are built with, and the context (adsb_create:
    two result sets of Seg entries, slots -- a tile's own and the pool --, list and channel prefix; the re-run plan and
    the exchange words)."""
    tiles, n_samples = len(c.perm), c.pool.iq.shape[1]
    tile = 16384                                              # the i8 scan's tile: the slot pool holds max_out + one tile
    samples = tiles * n_samples * 2 + c.pool.iq.nbytes + tiles * 8
    per_set = 16 * tiles + 24 * (tiles * FC.KQUOTA + max_out + tile) + 24 * max_out + 8 * (tiles + 1)
    words = (tiles // g.T + 2 + 63) // 64 * 64
    return samples + 2 * per_set + 4 * (tiles + 1) + 8 * (words + words // 64 + 64)


def test_big_shape_second_round_of_sums(gpu, oracle, g):
    import torch
    c = FC.case(oracle, I8, "big")
    workgroups = FC.shapes(g)["big"][0]
    assert (workgroups - 1) // g.F > g.S                      # the last workgroup reads more sums than one round holds
    max_out = int(c.prefix[-1]) + 64
    need = _big_bytes(g, c, max_out)
    free = torch.cuda.mem_get_info()[0]
    print(f"big: {len(c.perm)} channels, {need / GIB:.2f} GiB on the device ({free / GIB:.1f} GiB free)")
    if free < need + GIB:
        pytest.skip(f"{need / GIB:.2f} GiB + 1 GiB needed, {free / GIB:.2f} GiB free")
    assert free >= need
    iq = _device_input(c)
    with _ctx(c, max_out=max_out) as d:
        took = _check(d, iq, c, "big")
    print(f"big: {int(c.prefix[-1])} frames, two launches compared in {took:.2f} s")
    del iq


# ---- 5: the rebuild after a slot-pool overflow inside a two-level launch ---------------------------------------------------
def test_rebuild_inside_a_two_level_launch(gpu, oracle, g):
    base = FC.case(oracle, I8, "first")
    p = FC.with_constant(oracle, base.pool)
    constant = len(p.counts) - 1
    assert p.counts[constant] == FC.SAMPLES - FC.WINDOW > FC.KQUOTA            # every offset a frame: over the tile's slots
    perm = np.array(base.perm)
    where = (0, g.F * g.T, len(perm) - 1)                      # channel 0, the first tile of group 1, the last channel
    perm[list(where)] = constant
    c = FC.case_of(p, perm)
    assert all(c.counts[k] > FC.KQUOTA for k in where) and (np.delete(c.counts, where) <= FC.KQUOTA).all()
    iq = _device_input(c)
    with _ctx(c) as d:
        d.pool_limit(True)
        took = _check(d, iq, c, "rebuild")                     # flags == 0 after the fetch's rebuild
        d.pool_limit(False)
        _check(d, iq, c, "rebuild, pool on")
    print(f"rebuild: {int(c.prefix[-1])} frames, two launches compared in {took:.2f} s")
    del iq


# ---- 6: truncation ---------------------------------------------------------------------------------------------------------
def test_truncation_inside_a_channel(gpu, oracle, g):
    c = FC.case(oracle, I8, "first")
    mid = len(c.perm) // 2
    chan = mid + int(np.nonzero(c.counts[mid:] >= 2)[0][0])    # the first channel past the middle with two frames or more
    cut = int(c.prefix[chan]) + 1                              # its first frame is kept, its second is not
    assert c.prefix[chan] < cut < c.prefix[chan + 1] and 0.4 < cut / c.prefix[-1] < 0.6
    want_counts = FC.clipped_counts(c, cut)
    assert want_counts[chan] == 1 and not want_counts[chan + 1:].any() and want_counts.sum() == cut
    iq = _device_input(c)
    with _ctx(c, max_out=cut) as d:
        for run in range(2):
            frames, counts, total, flags = _launch(d, iq)
            assert flags == A.ADSB_FLAG_TRUNCATED, (run, flags)
            assert total == c.prefix[-1] and len(frames) == cut, (run, total, len(frames))
            _same_list(frames, c.frames[:cut], ("truncated", run))
            assert np.array_equal(np.asarray(counts, dtype=np.int64), want_counts), run
    del iq
