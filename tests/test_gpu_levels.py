"""Per-frame signal and noise power on the device (adsb_levels_device_async, adsb_fetch_levels, adsb_levels_of): the
integer records are compared == with the NumPy model (tests/levels_model.py) on the same IQ and the frames the launch
returned, for every shape a launch can have."""
import ctypes as C
import importlib.util
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import air_rs_amd as A
from air_rs_amd import _lib
from tests import finish_cases as FC
from tests import levels_cases as K
from tests import levels_model

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ZERO = np.zeros((), dtype=A.LEVEL_DTYPE).tobytes()


def _same(got, want):
    assert got.dtype.itemsize == want.dtype.itemsize == 32 and len(got) == len(want), (len(got), len(want))
    bad = [k for k in range(len(got)) if got[k].tobytes() != want[k].tobytes()]
    assert not bad, (bad[:5], got[bad[:3]], want[bad[:3]])


def _st(iq):
    return A.ADSB_SAMPLE_I8 if iq.dtype == np.int8 else A.ADSB_SAMPLE_I16


def _dev(arr):
    import torch
    return torch.from_numpy(np.ascontiguousarray(arr)).cuda()


# ---- 1: the fixtures, one-dispatch path and staged input -------------------------------------------------------------
@pytest.mark.parametrize("small", ["1", "0"])
def test_fixtures_through_demod(gpu, monkeypatch, small):
    monkeypatch.setenv("ADSB_SMALL_PATH", small)
    for name in K.FIXTURES:
        iq, want = K.fixture(name)
        with A.AdsbDemod(sample_type=_st(iq), max_samples=len(iq), max_out=4096) as d:
            frames, flags = d.demod(iq)
            assert flags == 0 and frames.tobytes() == want.tobytes(), name
            lv = d.levels()
            _same(lv, levels_model.levels(iq, frames))
            assert (lv["flags"] == A.ADSB_LEVEL_VALID).all() and len(lv) == len(frames) > 0, name
            if name == "ref_frames_i16":
                assert (lv["signal_sum"] == 9860000000).all()
            if name == "bit_errors_i8":
                assert (lv[0]["weak_bits"], lv[0]["pulse_min"], lv[0]["signal_sum"]) == (1, 5, 1127005)


# ---- 2: synthetic stream, both offset parities (the i8 window is dword-aligned only at even offsets) -----------------
@pytest.mark.parametrize("st", ["i8", "i16"])
def test_synthetic_both_parities(gpu, st):
    sample_type = A.ADSB_SAMPLE_I8 if st == "i8" else A.ADSB_SAMPLE_I16
    n = 3 * 16384 + 777
    iq = A.synth_fill_host(A.synth_default(seed=321, slot_len=500), sample_type, 0, 0, n)
    with A.AdsbDemod(sample_type=sample_type, max_samples=n, max_out=4096) as d:
        frames, flags = d.demod(iq)
        assert flags == 0 and len(frames) > 40
        assert set(int(o) % 2 for o in frames["offset"]) == {0, 1}
        _same(d.levels(), levels_model.levels(iq, frames))


# ---- 3: five channels, gaps of full-scale samples between them, and a stream base ------------------------------------
@pytest.mark.parametrize("base", [0, 10**12 + 1])
def test_multi_channel_with_stride_and_base(gpu, base):
    cfg = A.synth_default(seed=3, slot_len=800)
    nch, n = 5, 70_000 + 8
    stride = n + 8
    chans = [A.synth_fill_host(cfg, A.ADSB_SAMPLE_I8, c, 0, n) for c in range(nch)]
    buf = np.full((nch * stride, 2), -128, dtype=np.int8)          # the gaps: a wrong channel or stride shows as 32768
    for c in range(nch):
        buf[c * stride:c * stride + n] = chans[c]
    with A.AdsbDemod(max_samples=n, max_out=1 << 15, max_channels=nch, host_staging=False) as d:
        dev = _dev(buf)
        d.set_stream_base(base)
        d.demod_device_async(dev.data_ptr(), n, n_channels=nch, channel_stride=stride)
        d.levels_async()
        frames, counts, total, flags = d.fetch()
        assert flags == 0 and sum(counts) == len(frames) == total and min(counts) > 10
        lv = d.levels()
        assert len(lv) == len(frames)
        pos = 0
        for c in range(nch):
            part = frames[pos:pos + counts[c]]
            assert (part["offset"] >= base).all()
            _same(lv[pos:pos + counts[c]], levels_model.levels(chans[c], part, first_sample=base))
            pos += counts[c]
        del dev


# ---- 3b: more channels than one round of the channel lookup's ballot holds ------------------------------------------------
@pytest.mark.parametrize("nch", [64, 65, 66, 130])
def test_channel_lookup_past_one_ballot_round(gpu, oracle, nch):
    """frame_levels_kernel finds a frame's channel by counting, 64 channels per ballot, the channels that start at or
    before it in the list: 64 channels are one round with lane 63 idle, 65 fill it, 66 and 130 need a second and a third.
    One-tile channels of 1000 samples from the pool of tests/finish_cases.py, so every frame's window fits; channels
    without frames at the front, at index 64 and 65 and at the end (their prefix entries equal their neighbours')."""
    n = 1000
    p = FC.pool(oracle, A.ADSB_SAMPLE_I8, n)
    empty, full = np.nonzero(p.counts == 0)[0], np.nonzero(p.counts > 0)[0]
    rng = np.random.default_rng(nch)
    perm = full[rng.integers(0, len(full), nch)]
    for k, c in enumerate(c for c in (0, 64, 65, nch - 1) if c < nch):
        perm[c] = empty[k % len(empty)]
    c = FC.case_of(p, perm)
    assert c.counts[0] == c.counts[-1] == 0 and len(set(c.counts.tolist())) >= 4 and c.prefix[-1] > 4 * nch
    buf = np.ascontiguousarray(p.iq[perm])
    with A.AdsbDemod(max_samples=n, max_out=int(c.prefix[-1]) + 16, max_channels=nch, host_staging=False) as d:
        dev = _dev(buf)
        d.demod_device_async(dev.data_ptr(), n, n_channels=nch, channel_stride=n)
        frames, counts, total, flags = d.fetch()
        assert flags == 0 and total == len(frames) and frames.tobytes() == c.frames.tobytes()
        assert list(counts) == c.counts.tolist()
        lv = d.levels()
        assert len(lv) == len(frames) and (lv["flags"] == A.ADSB_LEVEL_VALID).all()
        for ch in range(nch):
            part = slice(int(c.prefix[ch]), int(c.prefix[ch + 1]))
            _same(lv[part], levels_model.levels(p.iq[perm[ch]], frames[part]))
        del dev


# ---- 4: full-scale pulses: p = 32768 (i8) and 2^31 (i16) -------------------------------------------------------------
@pytest.mark.parametrize("dt", [np.int8, np.int16], ids=["i8", "i16"])
def test_full_scale(gpu, dt):
    iq, planted, full = K.full_scale(dt)
    with A.AdsbDemod(sample_type=_st(iq), max_samples=len(iq), max_out=256) as d:
        frames, flags = d.demod(iq)
        assert flags == 0
        found = frames[np.isin(frames["offset"], K.FULL_SCALE_OFFSETS[:2])]
        assert len(found) == 2 and all(bytes(f["bytes"]) == K.FRAME for f in found)   # (the third ends on the last sample:
        lv = d.levels()                                                               #  no launch examines that offset)
        _same(lv, levels_model.levels(iq, frames))
        mine = lv[np.isin(frames["offset"], K.FULL_SCALE_OFFSETS[:2])]
        assert (mine["peak"] == full).all() and (mine["pulse_min"] == full).all()
        assert (mine["signal_sum"] == 116 * full).all() and (mine["weak_bits"] == 0).all()
        dev = _dev(iq)
        of = d.levels_of(dev.data_ptr(), len(iq), planted)
        _same(of, levels_model.levels(iq, planted))
        assert (of["peak"] == full).all() and (of["flags"] == 1).all()
        del dev


# ---- 5: fewer records asked for than frames found --------------------------------------------------------------------
def test_max_out_smaller_than_the_list(gpu):
    n = 60_000
    iq = A.synth_fill_host(A.synth_default(seed=9, slot_len=400), A.ADSB_SAMPLE_I8, 0, 0, n)
    with A.AdsbDemod(max_samples=n, max_out=4096) as d:
        frames, flags = d.demod(iq)
        assert len(frames) > 60
        want = levels_model.levels(iq, frames)
        _same(d.levels(max_out=17), want[:17])
        _same(d.levels(), want)
        # and a launch that keeps fewer frames than exist (max_out of the demod call)
        few, flags = d.demod(iq, max_out=40)
        assert flags & A.ADSB_FLAG_TRUNCATED and len(few) == 40
        _same(d.levels(max_out=40), want[:40])


# ---- 6: the list is rebuilt after a slot-pool overflow ---------------------------------------------------------------
def test_slot_pool_repair(gpu):
    cfg = A.synth_default(seed=19, slot_len=600)
    iq = A.synth_fill_host(cfg, A.ADSB_SAMPLE_I8, 0, 0, 300_000).copy()
    iq[40_000:95_000] = (3, 4)            # constant: one frame per offset, tiles far over their 32 slots
    iq[200_000:200_300] = 0
    with A.AdsbDemod(max_samples=300_000, max_out=1 << 18) as d:
        d.pool_limit(True)
        frames, flags = d.demod(iq)
        assert flags == 0 and len(frames) > 50_000
        want = levels_model.levels(iq, frames)
        _same(d.levels(), want)
        # device-resident launch: the levels are enqueued on the list with holes; the fetch's wait rebuilds the list
        # and the levels with it
        dev = _dev(iq)
        d.demod_device_async(dev.data_ptr(), len(iq))
        d.levels_async()
        lv = d.levels()
        d.pool_limit(False)
        again, _, _, flags = d.fetch()
        assert flags == 0 and again.tobytes() == frames.tobytes()
        _same(lv, want)
        del dev


# ---- 7: levels_of -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [np.int8, np.int16], ids=["i8", "i16"])
def test_levels_of(gpu, dt):
    st = A.ADSB_SAMPLE_I8 if dt == np.int8 else A.ADSB_SAMPLE_I16
    n = 20_000
    iq = A.synth_fill_host(A.synth_default(seed=77, slot_len=450), st, 0, 0, n)
    bad_iq, bad_frames, valid = K.invalid_list(dt)
    with A.AdsbDemod(sample_type=st, max_samples=n, max_out=4096) as d:
        frames, flags = d.demod(iq)
        assert flags == 0 and len(frames) > 20
        want = levels_model.levels(iq, frames)
        dev, dev_bad = _dev(iq), _dev(bad_iq)
        _same(d.levels_of(dev.data_ptr(), n, frames), want)                       # frames in host memory
        dev_frames = _dev(frames.view(np.uint8))
        _same(d.levels_of(dev.data_ptr(), n, (dev_frames.data_ptr(), len(frames))), want)   # in device memory
        # a slice of the buffer as a piece of a longer stream; frames before the slice become invalid
        cut, first = 1001, 123_456_789
        moved = frames.copy()
        moved["offset"] += np.uint64(first - cut)
        got = d.levels_of(dev.data_ptr() + cut * iq.itemsize * 2, n - cut, moved, first_sample=first)
        _same(got, levels_model.levels(iq[cut:], moved, first_sample=first))
        assert 0 < (got["flags"] == 0).sum() < len(got)
        assert got.tobytes() == A.host_frame_levels(iq[cut:], moved, first_sample=first).tobytes()
        # windows that do not fit: flags 0 and zeros, byte for byte what the CPU mirror gives
        got = d.levels_of(dev_bad.data_ptr(), len(bad_iq), bad_frames, first_sample=K.INVALID_FIRST)
        assert (got["flags"] == valid.astype(np.uint16)).all()
        assert all(got[k].tobytes() == ZERO for k in np.nonzero(~valid)[0])
        assert got.tobytes() == A.host_frame_levels(bad_iq, bad_frames, first_sample=K.INVALID_FIRST).tobytes()
        _same(got, levels_model.levels(bad_iq, bad_frames, first_sample=K.INVALID_FIRST))
        short = d.levels_of(dev_bad.data_ptr(), 239, K.frame_list([0, 1, 5000]))
        assert all(r.tobytes() == ZERO for r in short)
        assert len(d.levels_of(dev.data_ptr(), n, frames[:0])) == 0
        # none of it disturbed the last launch's levels
        _same(d.levels(), want)
        del dev, dev_bad, dev_frames


# ---- 8: state ---------------------------------------------------------------------------------------------------------
def test_state(gpu):
    L = _lib.load()
    n = 20_000
    iq1 = A.synth_fill_host(A.synth_default(seed=5, slot_len=450), A.ADSB_SAMPLE_I8, 0, 0, n)
    iq2 = A.synth_fill_host(A.synth_default(seed=6, slot_len=450), A.ADSB_SAMPLE_I8, 0, 0, n)
    out = (_lib.AdsbFrameLevel * 4096)()
    cnt, dev = C.c_size_t(), C.c_void_p()
    with A.AdsbDemod(max_samples=n, max_out=4096) as d:
        assert L.adsb_levels_device_async(d.handle) == A.ADSB_E_STATE           # before any launch
        assert L.adsb_fetch_levels(d.handle, out, 4096, C.byref(cnt)) == A.ADSB_E_STATE
        assert L.adsb_levels_device(d.handle, C.byref(dev)) == A.ADSB_E_STATE
        f1, _ = d.demod(iq1)
        assert L.adsb_fetch_levels(d.handle, out, 4096, C.byref(cnt)) == A.ADSB_E_STATE   # launched, nothing enqueued
        assert L.adsb_fetch_levels(d.handle, None, 4, C.byref(cnt)) == A.ADSB_E_ARG
        assert L.adsb_levels_of(d.handle, None, n, 0, None, 0, None) == A.ADSB_E_ARG
        _same(d.levels(), levels_model.levels(iq1, f1))
        assert L.adsb_levels_device(d.handle, C.byref(dev)) == A.ADSB_OK and dev.value == d.levels_device()
        f2, _ = d.demod(iq2)
        assert f2.tobytes() != f1.tobytes()
        assert L.adsb_fetch_levels(d.handle, out, 4096, C.byref(cnt)) == A.ADSB_E_STATE   # those were launch 1's
        _same(d.levels(), levels_model.levels(iq2, f2))                                    # levels() enqueues


# ---- 9: tools/replay.py --levels ---------------------------------------------------------------------------------------
def _db(total, n, full):
    return -math.inf if total == 0 else 10 * math.log10(total / n / full)


def test_replay_levels(gpu, oracle, tmp_path):
    from tests.golden.make_golden import REF_FRAMES, modulate, place
    chunk = 20_000
    items = [(chunk * (k // 3) + 300 + 2113 * (k % 3), modulate(bytes.fromhex(REF_FRAMES[k % 7]), (800 + 100 * k, 30), None))
             for k in range(12)]
    iq = place(chunk * 5, items, np.int16, floor=3, seed=5)        # (the fifth, frameless chunk is never sent)
    for j, v in enumerate(items[4][1]):                            # one packet between silent quiet samples: -inf
        if v is None:
            iq[items[4][0] + j] = 0
    path = tmp_path / "capture.c16"
    iq.astype("<i2").tofile(path)
    parts = []
    for c in range(4):                                             # what the replay decodes: every chunk on its own
        rc, fr, _ = oracle.process_buffer(iq[c * chunk:(c + 1) * chunk])
        assert rc == 0
        fr = fr.astype(K.FRAME_DTYPE)
        fr["offset"] += np.uint64(c * chunk)
        parts.append(fr)
    frames = np.concatenate(parts)
    assert [int(o) for o in frames["offset"]] == [o for o, _ in items]
    want = ""
    for f, lv in zip(frames, levels_model.levels(iq, frames)):
        sig, noise = _db(int(lv["signal_sum"]), 116, 2.0 ** 31), _db(int(lv["noise_sum"]), 124, 2.0 ** 31)
        icao = int.from_bytes(bytes(f["bytes"][1:4]), "big")
        want += f"{int(f['offset'])}\t{icao:x}\t{sig:.1f}\t{noise:.1f}\t{sig - noise:.1f}\t{int(lv['weak_bits'])}\n"
    assert want.count("\n") == 12 and want.count("-inf") == 1
    tool = os.path.join(ROOT, "tools", "replay.py")
    got = subprocess.run([sys.executable, tool, str(path), "--levels"], capture_output=True, text=True, timeout=300,
                         check=True).stdout
    assert got == want
    # the same text when the capture goes to the device in overlapping pieces
    spec = importlib.util.spec_from_file_location("replay_tool", tool)
    replay = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(replay)
    with A.AdsbDemod(sample_type=A.ADSB_SAMPLE_I16, max_samples=1024, max_out=64, host_staging=False) as d:
        assert replay.level_lines(d, A.ADSB_SAMPLE_I16, frames, iq, piece=7000) == want
