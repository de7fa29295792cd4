"""A real frame at every in-tile offset, through demod_tiles<I8>, demod_tiles<I16> and demod_small (tests/sweep_cases.py builds the
buffers; tests/test_sweep_cases.py shows on the CPU that the oracle's list of each is exactly what was planted).  The A/B scans
take the same sweep in tests/ab_cases.py::test_position_sweep.

The constant buffer reaches every in-tile offset and cannot see which sample a lane reads.  Here every in-tile offset carries a
frame of its own, at real (I, Q) samples, clean, with one flipped data bit or with every 0 bit a tie; the device's list must
equal the oracle's bit for bit, flags == 0:

  whole     each buffer in one launch through the three-kernel path: a dense and a sparse stride per sample type, CS16 again with
            a sample of root >= 31744 in every tile (the integer gate), i8 again with one sample and with half a tile + 5 dropped
            in front, and under each converter mode that ADSB_FORCE_MAG_MODE may force.
  slices    the same buffers cut at multiples of 32 tiles (in-tile offsets kept), one demod() per slice, against the oracle on
            that slice: through the one-dispatch path (ADSB_SMALL_PATH=1) and without it.
  channels  the same slices as the channels of one launch from device memory, 77s between the channels.

On a mismatch sweep_cases.compare names the first frames by tile and in-tile offset and the in-tile offsets concerned as ranges.
Every case prints samples, frames, survivors per tile, the oracle's seconds and its own (profiles/position_sweep_checks.txt)."""
import time

import numpy as np
import pytest

import air_rs_amd as A
from tests import sweep_cases as W

pytestmark = pytest.mark.gpu
ST = {"int8": A.ADSB_SAMPLE_I8, "int16": A.ADSB_SAMPLE_I16}
WHOLE = [n for n in W.CASES if not n.endswith("reg")]
SLICED = ["i8 dense", "i8 sparse", "cs16 dense", "cs16 sparse", "cs16 dense big", "cs16 sparse big"]
CAP = 1 << 16


def _line(name, what, s, frames, oracle_seconds, t0):
    per_tile = W.survivors_per_tile(s.mag, s.tile)
    print(f"\n{name}, {what}: {len(s.iq)} samples, {frames} frames, survivors per tile {per_tile.min()} .. {per_tile.max()}, "
          f"oracle {oracle_seconds:.2f} s, wall {time.perf_counter() - t0:.2f} s")


def _whole(oracle, name, what):
    t0 = time.perf_counter()
    s, want, seconds = W.reference(oracle, name)
    W.compare(want, s.planted, s.tile, name + ": the oracle against the plan")
    with A.AdsbDemod(sample_type=ST[s.iq.dtype.name], max_samples=len(s.iq), max_out=CAP) as d:
        frames, flags = d.demod(s.iq)
        mode = d.mag_mode
    assert flags == 0, (name, flags)
    W.compare(frames, want, s.tile, f"{name}, {what}")
    _line(name, what, s, len(frames), seconds, t0)
    return mode


@pytest.mark.parametrize("name", WHOLE)
def test_whole_buffer(gpu, oracle, monkeypatch, name):
    monkeypatch.delenv("ADSB_FORCE_MAG_MODE", raising=False)
    _whole(oracle, name, "whole")


@pytest.mark.parametrize("force", [1, 2])
def test_whole_buffer_under_a_forced_converter_mode(gpu, oracle, monkeypatch, force):
    # the modes tests/test_gpu_pair_dot.py forces: 0 is correct only where the converter truncates natively
    monkeypatch.setenv("ADSB_FORCE_MAG_MODE", str(force))
    assert _whole(oracle, "i8 dense", f"whole, converter mode {force}") == force


@pytest.mark.parametrize("small", ["1", "0"])
@pytest.mark.parametrize("name", SLICED)
def test_slices_of_32_tiles(gpu, oracle, monkeypatch, name, small):
    monkeypatch.delenv("ADSB_FORCE_MAG_MODE", raising=False)
    monkeypatch.setenv("ADSB_SMALL_PATH", small)
    t0 = time.perf_counter()
    s, _, seconds = W.reference(oracle, name)
    parts, _ = W.slice_reference(oracle, name)
    total = 0
    with A.AdsbDemod(sample_type=ST[s.iq.dtype.name], max_samples=W.SLICE_TILES * s.tile + W.WINDOW, max_out=CAP) as d:
        for j, (first, iq, want) in enumerate(parts):
            frames, flags = d.demod(iq)
            assert flags == 0, (name, j, flags)
            W.compare(frames, want, s.tile, f"{name}, slice {j} (from sample {first}), ADSB_SMALL_PATH={small}")
            total += len(frames)
    assert total == s.tile
    _line(name, f"{len(parts)} slices, ADSB_SMALL_PATH={small}", s, total, seconds, t0)


@pytest.mark.parametrize("name", SLICED)
def test_slices_as_channels(gpu, oracle, monkeypatch, name):
    import torch
    monkeypatch.delenv("ADSB_FORCE_MAG_MODE", raising=False)
    t0 = time.perf_counter()
    s, _, seconds = W.reference(oracle, name)
    parts, last = W.slice_reference(oracle, name)
    parts = parts[:-1] + [last]                                   # the ragged slice filled up: one length for all
    n = W.SLICE_TILES * s.tile + W.WINDOW
    stride = (n + 7) // 8 * 8 + 8                                 # a multiple of 8 samples
    host = np.full((len(parts), stride, 2), 77, dtype=s.iq.dtype)  # padding between channels must never be looked at
    for c, (_, iq, _) in enumerate(parts):
        assert len(iq) == n
        host[c, :n] = iq
    with A.AdsbDemod(sample_type=ST[s.iq.dtype.name], max_samples=n, max_out=CAP, max_channels=len(parts),
                     host_staging=False) as d:
        dev = torch.from_numpy(host).cuda()
        torch.cuda.synchronize()
        d.demod_device_async(dev.data_ptr(), n, len(parts), stride)
        frames, counts, total, flags = d.fetch(n_channels=len(parts))
    assert flags == 0 and total == len(frames) == sum(len(w) for _, _, w in parts), (name, flags, total, len(frames))
    assert total >= s.tile
    pos = 0
    for c, (first, _, want) in enumerate(parts):
        assert counts[c] == len(want), (name, c, counts[c], len(want))
        W.compare(frames[pos:pos + len(want)], want, s.tile, f"{name}, channel {c} (from sample {first})")
        pos += len(want)
    _line(name, f"{len(parts)} channels", s, total, seconds, t0)
