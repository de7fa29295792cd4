"""The wire-input model (tests/wire_in_model.py) with ADSB_WIRE_IN_SHORT: the old model's framing -- its marks, its reader
of one mark, its consumed rule -- plus the emission of the complete 56-bit frames (Beast '2', '*' with 14 digits, '@' with
26).  Without the bit it is the old model itself.  Calls no library entry point."""
import numpy as np

from tests import wire_in_model as M
from tests.wire_model import FRAME_DTYPE, LEVEL_DTYPE, I8, BEAST, smallest_sum_for

SHORT = 4


def beast_events(B):
    """One stream -> (events, consumed, counters) with a '2' frame an event like a '3' frame; n_other counts '1' only."""
    events, c = [], dict(n_marks=0, n_cut=0, n_unknown=0, n_other=0)
    incomplete, last_end = None, 0
    for m in M.beast_marks(B):
        c["n_marks"] += 1
        state, end, out = M.read_beast(B, m)
        if state == "unknown":
            c["n_unknown"] += 1
        elif state == "cut":
            c["n_cut"] += 1
        elif state == "incomplete":
            incomplete = m
        else:
            last_end = end
            if B[m + 1] in (0x32, 0x33):
                events.append((m, int.from_bytes(out[:6], "big"), out[6], B[m + 1], out[7:]))
            else:
                c["n_other"] += 1
    N = len(B)
    if incomplete is not None:
        consumed = incomplete
    else:
        k = 0
        while k < N and B[N - 1 - k] == 0x1A and N - 1 - k >= last_end:
            k += 1
        consumed = N - k % 2
    return events, consumed, c


def avr_events(B):
    events, c = [], dict(n_marks=0, n_cut=0, n_unknown=0, n_other=0)
    N, consumed = len(B), len(B)
    for p in range(N):
        if B[p] not in b"*@":
            continue
        c["n_marks"] += 1
        star, h = B[p] == 0x2A, 0
        while h < 41 and p + 1 + h < N and B[p + 1 + h] in M.HEX:
            h += 1
        after = p + 1 + h
        if h < 41 and after < N and B[after] == 0x3B:
            digits = B[p + 1:after].decode()
            stamp = 0 if star else 12
            if h - stamp in (28, 14):
                t = int(digits[:12], 16) if stamp else 0
                events.append((p, t, 0, B[p], bytes.fromhex(digits[stamp:])))
            elif h - stamp == 4:
                c["n_other"] += 1
            else:
                c["n_cut"] += 1
        elif after == N and h <= (28 if star else 40):
            consumed = p
        else:
            c["n_cut"] += 1
    return events, consumed, c


def keeps(filter, msg):
    if len(msg) == 14:
        return M.keeps(filter & 3, msg)
    if filter & M.DF17:
        return False
    return not (filter & M.CRC and M.crc24(msg[:4]) ^ int.from_bytes(msg[4:7], "big"))


def parse(stream, stream_ends=None, fmt=BEAST, filter=0, tick_bias=0, max_frames=0, sample_type=I8, levels=False):
    """As wire_in_model.parse; with SHORT in `filter` the short frames are in the list."""
    if not filter & SHORT:
        return M.parse(stream, stream_ends, fmt, filter, tick_bias, max_frames, sample_type, levels)
    stream = bytes(stream)
    ends = [len(stream)] if stream_ends is None else [int(e) for e in stream_ends]
    most = len(stream) // 16
    cap = most if not max_frames else min(int(max_frames), most)
    header = dict.fromkeys(M.HEADER_FIELDS, 0)
    rows, counts, consumed, start = [], [], [], 0
    for r, end in enumerate(ends):
        events, used, c = (beast_events if fmt == BEAST else avr_events)(stream[start:end])
        for k, v in c.items():
            header[k] += v
        before = min(len(rows), cap)
        for ev in events:
            if keeps(filter, ev[4]):
                rows.append((r,) + ev)
            else:
                header["n_rejected"] += 1
        counts.append(min(len(rows), cap) - before)
        consumed.append(used)
        start = end
    header["total_found"], header["n_frames"] = len(rows), min(len(rows), cap)
    header["flags"] = M.TRUNCATED if len(rows) > cap else 0
    rows = rows[:cap]
    fr, rx = np.zeros(len(rows), dtype=FRAME_DTYPE), np.zeros(len(rows), dtype=M.RX_DTYPE)
    lv = np.zeros(len(rows), dtype=LEVEL_DTYPE) if levels else None
    for i, (r, pos, t, s, kind, msg) in enumerate(rows):
        fr[i] = (((t - tick_bias) % (1 << 48)) // 6, np.frombuffer(msg.ljust(14, b"\0"), dtype=np.uint8), 0, 0xFF)
        rx[i] = (t, pos, s, kind, r)
        if levels and s:
            lv[i]["signal_sum"], lv[i]["flags"] = smallest_sum_for(s, sample_type), 1
    return dict(frames=fr, rx=rx, levels=lv, counts=np.array(counts, dtype=np.uint64),
                consumed=np.array(consumed, dtype=np.uint64), header=header)


# ---- streams -------------------------------------------------------------------------------------------------------------
def beast_frame(kind, t, s, msg):
    body = int(t).to_bytes(6, "big") + bytes([s]) + bytes(msg)
    return b"\x1a" + kind + body.replace(b"\x1a", b"\x1a\x1a")


def avr_line(msg, t=None, upper=True, eol=b"\n"):
    text = bytes(msg).hex()
    text = text.upper() if upper else text
    return (b"*" if t is None else b"@" + b"%012X" % t) + text.encode() + b";" + eol


def mixed_beast(rng, n, one_in=6):
    """n frames of types '1', '2', '3' (half of them short) with one byte in `one_in` 0x1A, timestamp and signal too ->
    (stream, the frames' ends)."""
    parts = []
    for _ in range(n):
        kind = (b"2", b"2", b"3", b"1")[int(rng.integers(0, 4))]
        size = {b"1": 2, b"2": 7, b"3": 14}[kind]
        raw = rng.integers(0, 256, size=7 + size)
        raw[rng.integers(0, one_in, size=7 + size) == 0] = 0x1A
        parts.append(beast_frame(kind, int.from_bytes(bytes(raw[:6].astype(np.uint8)), "big"), int(raw[6]),
                                 bytes(raw[7:].astype(np.uint8))))
    return b"".join(parts), np.cumsum([len(p) for p in parts])


def mixed_avr(rng, n):
    """n lines over all six AVR shapes, in either case, with '\\n' or '\\r\\n'"""
    parts = []
    for _ in range(n):
        size = (2, 7, 14)[int(rng.integers(0, 3))]
        msg = bytes(rng.integers(0, 256, size=size).astype(np.uint8))
        t = None if rng.integers(0, 2) else int(rng.integers(0, 1 << 48))
        parts.append(avr_line(msg, t, bool(rng.integers(0, 2)), (b"\n", b"\r\n")[int(rng.integers(0, 2))]))
    return b"".join(parts), np.cumsum([len(p) for p in parts])
