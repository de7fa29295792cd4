"""A frame at every offset around every seam of a time-sharded buffer (tests/seam_cases.py; tests/test_seam_cases.py
shows on the CPU that the oracle's list holds them): through adsb_group_* from a host buffer and from slices of one
device buffer, through sharding.plan with one context per shard, with fewer offsets than members, with the output
capacity running out exactly at a seam, and with every member's slice generated on the device by itself.  Every list is
compared == with the oracle's over the whole buffer, and its offsets ascend strictly: no frame lost, none twice."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import air_rs_amd as A
from air_rs_amd import sharding
from tests import seam_cases as S
from tests.test_gpu_round2 import _eq

pytestmark = pytest.mark.gpu
CAP = 1 << 14


def _whole(frames, want):
    assert (np.diff(frames["offset"].astype(np.int64)) > 0).all()
    _eq(frames, want)


def _slices(tensor, plan, bps):
    return [tensor.data_ptr() + first * bps if ns else None for first, ns, noff in plan]


@pytest.mark.parametrize("t", S.TYPES)
@pytest.mark.parametrize("world", S.WORLDS)
def test_seams_through_a_group(gpu, oracle, world, t):
    import torch
    st, bps = S.TYPES[t], 2 if t == "i8" else 4
    with A.AdsbGroup([0] * world, sample_type=st, max_samples=S.total_of(world, max(S.RAGGED)), max_out=CAP) as g:
        for r in S.RAGGED:
            total = S.total_of(world, r)
            iq, want, seams = S.seam_buffer(oracle, st, total, world)
            assert len(seams) == world - 1 and (world - 1) * 601 <= len(want) < CAP
            frames, flags = g.demod(iq)                       # host buffer -> per-member copies -> launches -> merge
            assert flags == 0, (r, flags)
            _whole(frames, want)
            dev = torch.from_numpy(iq.copy()).cuda()          # slices of ONE device buffer
            torch.cuda.synchronize()
            g.demod_device_async(_slices(dev, A.group_plan(total, world), bps), total)
            frames, found, flags = g.fetch()
            assert flags == 0 and found == len(want), (r, flags, found)
            _whole(frames, want)


@pytest.mark.parametrize("t", S.TYPES)
def test_fewer_offsets_than_members(gpu, t):
    import torch
    st, bps = S.TYPES[t], 2 if t == "i8" else 4
    with A.AdsbGroup([0] * 8, sample_type=st, max_samples=A.WINDOW + max(S.FEW), max_out=64) as g:
        for k in S.FEW:
            iq = S.few_offsets_buffer(st, k)
            plan = A.group_plan(len(iq), 8)
            assert not any(noff for first, ns, noff in plan[3:])
            frames, flags = g.demod(iq)
            assert flags == 0 and len(frames) == k
            assert (frames["offset"] == np.arange(k)).all() and not frames["bytes"].any() and not frames["status"].any()
            dev = torch.from_numpy(iq).cuda()
            torch.cuda.synchronize()
            g.demod_device_async(_slices(dev, plan, bps), len(iq))
            again, found, flags = g.fetch()
            assert flags == 0 and found == k
            _eq(again, frames)


@pytest.mark.parametrize("t", S.TYPES)
def test_truncation_at_a_seam(gpu, oracle, t):
    import torch
    st, bps, world = S.TYPES[t], 2 if t == "i8" else 4, 3
    total = S.total_of(world, 7)
    iq, want, seams = S.seam_buffer(oracle, st, total, world)
    plan = A.group_plan(total, world)
    c0 = int((want["offset"] < plan[1][0]).sum())            # member 0's frames
    assert 300 <= c0 < len(want) - 600 and want["offset"][c0] == seams[0]
    dev = torch.from_numpy(iq.copy()).cuda()
    torch.cuda.synchronize()
    for cap in (c0 - 1, c0, c0 + 1):
        with A.AdsbGroup([0] * world, sample_type=st, max_samples=total, max_out=cap, host_staging=False) as g:
            g.demod_device_async(_slices(dev, plan, bps), total)
            frames, found, flags = g.fetch()
            assert flags & A.ADSB_FLAG_TRUNCATED and found == len(want), (cap, flags, found)
            _whole(frames, want[:cap])


@pytest.mark.parametrize("t", S.TYPES)
@pytest.mark.parametrize("world", S.WORLDS)
def test_seams_through_the_python_plan(gpu, oracle, world, t):
    """sharding.plan run shard after shard, one context per shard, each with adsb_set_stream_base(first sample of its
    slice): the per-shard lists, merely concatenated, are the oracle's list."""
    st = S.TYPES[t]
    biggest = max(sh.n_samples for sh in sharding.plan(S.total_of(world, max(S.RAGGED)), world))
    with contextlib.ExitStack() as stack:
        dems = [stack.enter_context(A.AdsbDemod(sample_type=st, max_samples=biggest, max_out=CAP)) for _ in range(world)]
        for r in S.RAGGED:
            total = S.total_of(world, r)
            iq, want, seams = S.seam_buffer(oracle, st, total, world)
            parts = []
            for d, sh in zip(dems, sharding.plan(total, world)):
                assert sh.n_samples == sh.n_offsets + A.WINDOW > A.WINDOW
                d.set_stream_base(sh.first_sample)
                fr, fl = d.demod(iq[sh.first_sample: sh.first_sample + sh.n_samples])
                assert fl == 0
                assert len(fr) and fr["offset"][0] >= sh.first_offset and fr["offset"][-1] < sh.first_offset + sh.n_offsets
                parts.append(fr)
            _whole(np.concatenate(parts), want)
            _whole(sharding.merge_rank_lists([(len(p), len(p), 0, p) for p in parts]), want)


@pytest.mark.parametrize("t", S.TYPES)
@pytest.mark.parametrize("slot_len", [2000, 256])
@pytest.mark.parametrize("world", S.WORLDS)
def test_device_generated_slices_join_into_one_stream(gpu, oracle, world, slot_len, t):
    """Every member generates its own slice (adsb_synth_fill_device on its context, absolute sample numbers) into an
    allocation of its own; the group's list is the oracle's over the host fill of the whole range.  slot_len 2000 is the
    default config; 256 puts a frame every 256 samples, so frames straddle every seam."""
    import torch
    st, bps = S.TYPES[t], 2 if t == "i8" else 4
    cfg = A.synth_default() if slot_len == 2000 else A.synth_default(slot_len=slot_len)
    lib = A.load()
    with A.AdsbGroup([0] * world, sample_type=st, max_samples=S.total_of(world, max(S.RAGGED)), max_out=CAP,
                     host_staging=False) as g:
        for r in S.RAGGED:
            total = S.total_of(world, r)
            whole = A.synth_fill_host(cfg, st, 0, 0, total)
            rc, want, found = oracle.process_buffer(whole)
            assert rc == 0 and len(want) >= total // slot_len // 2
            plan = A.group_plan(total, world)
            bufs = [torch.empty(ns * bps, dtype=torch.uint8, device="cuda") for first, ns, noff in plan]
            torch.cuda.synchronize()
            for i, (first, ns, noff) in enumerate(plan):
                member = lib.adsb_group_member(g._h, i)
                assert member and ns == noff + A.WINDOW
                assert lib.adsb_synth_fill_device(member, C.byref(cfg), 0, first, ns, bufs[i].data_ptr()) == A.ADSB_OK
            g.demod_device_async([b.data_ptr() for b in bufs], total)
            frames, found, flags = g.fetch()
            assert flags == 0 and found == len(want)
            _whole(frames, want)
            torch.cuda.synchronize()
            for b, (first, ns, noff) in zip(bufs, plan):
                assert (b.cpu().numpy() == whole[first:first + ns].view(np.uint8).reshape(-1)).all()
