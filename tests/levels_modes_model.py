"""NumPy model of the level records by frame length (include/adsb_hip.h, "Level records by frame length"), written from
the header's definition: a frame's length from its DF, the window, the pulse set, the six statistics.  Also the signal
byte of such a record by search over s, and the wire bytes of a mixed list put together from
tests/wire_in_short_model.py's encoder.  Calls no library entry point; its dtypes are written out here."""
import functools

import numpy as np

from tests.wire_in_short_model import avr_line, beast_frame

MODEL_DTYPE = np.dtype([("signal_sum", "<u8"), ("noise_sum", "<u8"), ("peak", "<u4"), ("pulse_min", "<u4"),
                        ("quiet_max", "<u4"), ("weak_bits", "<u2"), ("flags", "<u2")])
FRAME_DTYPE = np.dtype([("offset", "<u8"), ("bytes", "u1", (14,)), ("status", "u1"), ("fixed_bit", "u1")])
VALID, SHORT = 1, 2
FULL_SCALE = {0: 32768, 1: 1 << 31}
PREAMBLE = (0, 2, 7, 9)


def n_bits(frame_bytes):
    """56 for a DF below 16, else 112"""
    return 56 if (int(frame_bytes[0]) >> 3) < 16 else 112


def one(p, w, frame_bytes):
    """the record of a frame at sample w of a channel whose powers are p (a Python list / int64 array)"""
    bits = n_bits(frame_bytes)
    window = 16 + 2 * bits
    rec = np.zeros((), dtype=MODEL_DTYPE)
    if w < 0 or w + window > len(p):
        return rec
    value = int.from_bytes(bytes(frame_bytes[:bits // 8]), "big")
    pulse, weak = set(PREAMBLE), 0
    for b in range(bits):
        bit = value >> (bits - 1 - b) & 1
        hi, lo = (16 + 2 * b, 17 + 2 * b) if bit else (17 + 2 * b, 16 + 2 * b)
        pulse.add(hi)
        weak += int(p[w + hi]) < 2 * int(p[w + lo])
    loud = [int(p[w + k]) for k in sorted(pulse)]
    quiet = [int(p[w + k]) for k in range(window) if k not in pulse]
    assert len(loud) == 4 + bits and len(quiet) == 12 + bits
    rec["signal_sum"], rec["noise_sum"] = sum(loud), sum(quiet)
    rec["peak"], rec["pulse_min"], rec["quiet_max"] = max(loud + quiet), min(loud), max(quiet)
    rec["weak_bits"], rec["flags"] = weak, VALID | (SHORT if bits == 56 else 0)
    return rec


def levels(iq, frames, counts=None, n_samples=None, channel_stride=None, first_sample=0):
    """One MODEL_DTYPE record per frame.  iq: the flat (samples, 2) buffer; counts[c] frames belong to channel c, which is
    the n_samples samples from c x channel_stride."""
    flat = np.asarray(iq).reshape(-1, 2).astype(np.int64)
    power = flat[:, 0] ** 2 + flat[:, 1] ** 2
    counts = [len(frames)] if counts is None else [int(c) for c in counts]
    n_samples = len(power) // len(counts) if n_samples is None else n_samples
    stride = n_samples if channel_stride is None else channel_stride
    assert sum(counts) == len(frames)
    out, i = np.zeros(len(frames), dtype=MODEL_DTYPE), 0
    for c, k in enumerate(counts):
        p = power[c * stride:c * stride + n_samples]
        for _ in range(k):
            out[i] = one(p, int(frames["offset"][i]) - int(first_sample), frames["bytes"][i])
            i += 1
    return out


def signal_byte(level, sample_type, short_flag=True):
    """The signal byte of a record by definition: the largest s in 0..255 with (2s-1)^2 x P x FS <= 4 x 255^2 x sum, at
    least 1 for a sum above zero; P = 60 for a SHORT record when the format has the short bit, else 116."""
    if level is None or not int(level["flags"]) & VALID:
        return 0
    total = int(level["signal_sum"])
    if total == 0:
        return 0
    return _search(total, 60 if short_flag and int(level["flags"]) & SHORT else 116, FULL_SCALE[sample_type])


@functools.lru_cache(maxsize=None)
def _search(total, pulses, full_scale):
    best = 0
    for s in range(1, 256):
        if (2 * s - 1) ** 2 * pulses * full_scale <= 4 * 255 * 255 * total:
            best = s
    return max(best, 1)


def encode(fmt, frames, levels=None, sample_type=0, tick_bias=0):
    """(stream, ends as uint32) of a list with the short bit set: Beast '2' / '3', '*' and '@' lines with 14 or 28 digits"""
    out, ends = bytearray(), []
    for i, f in enumerate(frames):
        msg = bytes(f["bytes"][:n_bits(f["bytes"]) // 8])
        t = (6 * int(f["offset"]) + int(tick_bias)) % (1 << 48)
        if fmt == "beast":
            s = signal_byte(levels[i], sample_type) if levels is not None else 0
            out += beast_frame(b"2" if len(msg) == 7 else b"3", t, s, msg)
        else:
            out += avr_line(msg, t if fmt == "avr_mlat" else None)
        ends.append(len(out))
    return bytes(out), np.array(ends, dtype=np.uint32)


def signal_bytes(levels, sample_type):
    return [signal_byte(lv, sample_type) for lv in levels]
