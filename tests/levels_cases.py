"""Inputs shared by the CPU and GPU tiers of the per-frame level tests: golden fixtures, hand-modulated full-scale frames,
and a frame list with windows that do not fit their buffer."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = ("ref_frames_i8", "ref_frames_i16", "bit_errors_i8", "len241_i8", "sqrt_ties_i8")
FRAME = bytes.fromhex("8d406b902015a678d4d220aa4bda")          # a frame of the reference's own tests (CRC good)
FRAME_DTYPE = np.dtype([("offset", "<u8"), ("bytes", "u1", (14,)), ("status", "u1"), ("fixed_bit", "u1")])


def fixture(name):
    z = np.load(os.path.join(HERE, "golden", name + ".npz"), allow_pickle=False)
    return z["iq"], z["frames"].astype(FRAME_DTYPE)


def frame_list(offsets, frame=FRAME):
    fr = np.zeros(len(offsets), dtype=FRAME_DTYPE)
    fr["offset"] = np.array(offsets, dtype=np.uint64)
    fr["bytes"] = np.frombuffer(frame, dtype=np.uint8)
    fr["fixed_bit"] = 0xFF
    return fr


def modulate(iq, start, hi, frame=FRAME):
    """Writes the 116 pulse samples of `frame` at window `start` of iq as (I, Q) = hi; the quiet samples stay."""
    for p in (0, 2, 7, 9):
        iq[start + p] = hi
    bits = np.unpackbits(np.frombuffer(frame, dtype=np.uint8))
    for b in range(112):
        iq[start + 16 + 2 * b + (0 if bits[b] else 1)] = hi
    return iq


FULL_SCALE_OFFSETS = (100, 501, 960)    # both parities; the last window ends on the buffer's last sample


def full_scale(dtype):
    """(iq, frames, full-scale power): three frames whose pulses are the most negative sample, (-128, -128) or
    (-32768, -32768), on a floor of +-3; p = 32768 or 2^31, which int32 does not hold."""
    lo = int(np.iinfo(dtype).min)
    rng = np.random.default_rng(11)
    iq = rng.integers(-3, 4, size=(1200, 2)).astype(dtype)
    for off in FULL_SCALE_OFFSETS:
        modulate(iq, off, (lo, lo))
    return iq, frame_list(FULL_SCALE_OFFSETS), 2 * lo * lo


INVALID_FIRST = 5000


def invalid_list(dtype):
    """(iq of 1000 samples whose sample 0 is stream sample 5000, frames, which of them are valid).  Invalid: windows
    past the end (by one sample, by far, offset near 2^64) and offsets before the buffer's first sample."""
    rng = np.random.default_rng(12)
    top = 100 if dtype == np.int8 else 20000
    iq = rng.integers(-top, top + 1, size=(1000, 2)).astype(dtype)
    f = INVALID_FIRST
    offsets = [f, f + 1, f + 759, f + 760, f + 761, f + 1000, f - 1, 0, 239, (1 << 64) - 1, 1 << 63, f + 333]
    valid = [True, True, True, True, False, False, False, False, False, False, False, True]
    return iq, frame_list(offsets), np.array(valid)
