"""Independent model of the wire output (include/adsb_hip.h, "Wire output"): an encoder written from the format's
definition with Python integers, and a parser that takes a stream apart again.  Shared by the CPU and GPU tiers; also
the hand-made frame lists both use."""
import math

import numpy as np

FRAME_DTYPE = np.dtype([("offset", "<u8"), ("bytes", "u1", (14,)), ("status", "u1"), ("fixed_bit", "u1")])
LEVEL_DTYPE = np.dtype([("signal_sum", "<u8"), ("noise_sum", "<u8"), ("peak", "<u4"), ("pulse_min", "<u4"),
                        ("quiet_max", "<u4"), ("weak_bits", "<u2"), ("flags", "<u2")])
BEAST, AVR, AVR_MLAT = "beast", "avr", "avr_mlat"
FORMATS = (BEAST, AVR, AVR_MLAT)
I8, I16 = 0, 1
FULL_SCALE = {I8: 32768, I16: 1 << 31}
KNOWN = bytes.fromhex("8D4840D6202CC371C32CE0576098")
ALL_1A = bytes([0x1A] * 14)
ALL_1A_OFFSET = 0x1A1A1A1A1A1A // 6      # 6 x this is 0x1A1A1A1A1A1A exactly: every timestamp byte is 0x1A


def ticks(offset, tick_bias=0):
    return (6 * int(offset) + int(tick_bias)) % (1 << 48)


def signal_byte_by_definition(signal_sum, sample_type):
    """The largest s in 0..255 with (2s-1)^2 116 FS <= 4 255^2 sum; 0 only for a sum of 0."""
    signal_sum = int(signal_sum)
    if signal_sum == 0:
        return 0
    unit = 116 * FULL_SCALE[sample_type]
    best = 0
    for s in range(1, 256):
        if (2 * s - 1) ** 2 * unit <= 4 * 255 * 255 * signal_sum:
            best = s
    return max(best, 1)


def signal_byte(signal_sum, sample_type):
    """The same in closed form, for long lists: (2s-1)^2 <= floor(4 255^2 sum / (116 FS)), so 2s-1 <= its integer
    root.  tests/test_wire_host.py holds it to the definition at every boundary."""
    signal_sum = int(signal_sum)
    if signal_sum == 0:
        return 0
    root = math.isqrt(4 * 255 * 255 * signal_sum // (116 * FULL_SCALE[sample_type]))
    return max(min((root + 1) // 2, 255), 1)


def smallest_sum_for(s, sample_type):
    """The smallest signal_sum that gives signal byte s >= 2 (s = 1: the sum 1): ceil((2s-1)^2 116 FS / (4 255^2))."""
    if s == 1:
        return 1
    num, den = (2 * s - 1) ** 2 * 116 * FULL_SCALE[sample_type], 4 * 255 * 255
    return -(-num // den)


def level_signal(level, sample_type):
    if level is None or not (int(level["flags"]) & 1):
        return 0
    return signal_byte(level["signal_sum"], sample_type)


def encode_one(fmt, offset, frame14, s=0, tick_bias=0):
    t = ticks(offset, tick_bias)
    frame14 = bytes(frame14)
    assert len(frame14) == 14
    if fmt == BEAST:
        payload = t.to_bytes(6, "big") + bytes([s]) + frame14
        return b"\x1a\x33" + payload.replace(b"\x1a", b"\x1a\x1a")
    if fmt == AVR:
        return b"*" + frame14.hex().upper().encode() + b";\n"
    assert fmt == AVR_MLAT
    return b"@" + b"%012X" % t + frame14.hex().upper().encode() + b";\n"


def encode(fmt, frames, levels=None, sample_type=I8, tick_bias=0):
    """(stream, ends) of a FRAME_DTYPE list with its LEVEL_DTYPE list (None: no signal byte)."""
    out, ends = bytearray(), []
    for i, f in enumerate(frames):
        s = level_signal(levels[i], sample_type) if levels is not None and fmt == BEAST else 0
        out += encode_one(fmt, f["offset"], f["bytes"].tobytes(), s, tick_bias)
        ends.append(len(out))
    return bytes(out), np.array(ends, dtype=np.uint32)


def parse(fmt, stream):
    """The stream back to [(t, s, frame bytes)]; t is None for plain AVR and s is None for both AVR forms.  Asserts
    the framing on the way."""
    out, p = [], 0
    while p < len(stream):
        if fmt == BEAST:
            assert stream[p:p + 2] == b"\x1a\x33", (p, stream[p:p + 2])
            p += 2
            body = bytearray()
            while len(body) < 21:
                b = stream[p]
                p += 1
                if b == 0x1A:
                    assert stream[p] == 0x1A, p      # a lone 0x1A inside a message would start the next one
                    p += 1
                body.append(b)
            out.append((int.from_bytes(body[:6], "big"), body[6], bytes(body[7:])))
        else:
            n = 31 if fmt == AVR else 43
            line = stream[p:p + n]
            assert len(line) == n and line[-2:] == b";\n" and line[:1] == (b"*" if fmt == AVR else b"@"), line
            digits = line[1:-2].decode()
            assert digits == digits.upper()
            t = None if fmt == AVR else int(digits[:12], 16)
            out.append((t, None, bytes.fromhex(digits[-28:])))
            p += n
    return out


def expected_parse(fmt, frames, levels=None, sample_type=I8, tick_bias=0):
    """What parse() of a correct stream returns."""
    out = []
    for i, f in enumerate(frames):
        s = level_signal(levels[i], sample_type) if levels is not None else 0
        out.append((None if fmt == AVR else ticks(f["offset"], tick_bias), s if fmt == BEAST else None,
                    f["bytes"].tobytes()))
    return out


def split(stream, ends):
    """The stream cut at ends[]: one bytes object per frame."""
    cuts = [0] + [int(e) for e in ends]
    return [stream[a:b] for a, b in zip(cuts, cuts[1:])]


def whole_frames(ends, cap):
    """Bytes of the longest prefix of whole frames that fits cap."""
    fit = [int(e) for e in ends if int(e) <= cap]
    return fit[-1] if fit else 0


# ---- frame lists --------------------------------------------------------------------------------------------------------
def frame_list(offsets, frames14):
    fr = np.zeros(len(offsets), dtype=FRAME_DTYPE)
    fr["offset"] = np.array([int(o) % (1 << 64) for o in offsets], dtype=np.uint64)
    for k, b in enumerate(frames14):
        fr["bytes"][k] = np.frombuffer(bytes(b), dtype=np.uint8)
    fr["fixed_bit"] = 0xFF
    return fr


def level_list(sums, flags=1):
    lv = np.zeros(len(sums), dtype=LEVEL_DTYPE)
    lv["signal_sum"] = np.array([int(s) for s in sums], dtype=np.uint64)
    lv["flags"] = flags
    return lv


def random_frames(n, seed, one_in=8):
    """n frames at ascending offsets whose bytes are 0x1A with probability 1 / one_in (and whose timestamps hold 0x1A
    now and then): lengths vary, so workgroup spans start at every alignment."""
    rng = np.random.default_rng(seed)
    fr = np.zeros(n, dtype=FRAME_DTYPE)
    fr["offset"] = np.cumsum(rng.integers(1, 3000, size=n)).astype(np.uint64)
    b = rng.integers(0, 256, size=(n, 14)).astype(np.uint8)
    b[rng.integers(0, one_in, size=(n, 14)) == 0] = 0x1A
    fr["bytes"] = b
    fr["status"] = rng.integers(0, 2, size=n)
    return fr


def random_levels(n, seed, sample_type=I8):
    """Level records whose signal bytes cover 0..255, a few of them invalid."""
    rng = np.random.default_rng(seed)
    top = 116 * FULL_SCALE[sample_type]
    lv = np.zeros(n, dtype=LEVEL_DTYPE)
    lv["signal_sum"] = (rng.random(n) ** 2 * top).astype(np.uint64)
    lv["noise_sum"] = rng.integers(0, 1000, size=n)
    lv["flags"] = (rng.integers(0, 16, size=n) != 0).astype(np.uint16)
    return lv


def all_1a_frame():
    """(frames, levels): the frame whose 21 payload bytes are all 0x1A (44 bytes of Beast), i8 full scale."""
    s26 = smallest_sum_for(26, I8)
    assert signal_byte(s26, I8) == 26 == 0x1A
    return frame_list([ALL_1A_OFFSET], [ALL_1A]), level_list([s26])


def plain_frame(offset):
    """A frame without a single 0x1A at an offset whose timestamp has none either: 23 bytes of Beast."""
    return frame_list([offset], [KNOWN])
