"""Independent sequential model of the wire input (include/adsb_hip.h, "Wire input"), written from the definitions over
Python bytes: marks by the parity of maximal 0x1A runs, the reader of one mark, `consumed` from the complete frames'
ends, the AVR candidates, the filters (CRC-24 from the generator) and the capacity rule.  Calls no library entry point.
Shared by the CPU and GPU tiers, with the comparison of a library result against it."""
import numpy as np

from tests.wire_model import (FRAME_DTYPE, LEVEL_DTYPE, I8, I16, BEAST, AVR, AVR_MLAT, encode, random_frames,  # noqa: F401
                              random_levels, smallest_sum_for)

RX_DTYPE = np.dtype([("ticks", "<u8"), ("pos", "<u4"), ("signal", "u1"), ("kind", "u1"), ("receiver", "<u2")])
HEADER_FIELDS = ("n_frames", "total_found", "n_marks", "n_cut", "n_unknown", "n_other", "n_rejected", "flags")
CRC, DF17 = 1, 2
TRUNCATED = 1
LENGTHS = {0x31: 2, 0x32: 7, 0x33: 14}
HEX = b"0123456789abcdefABCDEF"
GENERATOR = 0x1FFF409


def crc24(data):
    """Mode-S CRC-24: the remainder of data x 2^24 by the generator, by long division."""
    v = int.from_bytes(bytes(data), "big") << 24
    for i in range(v.bit_length() - 1, 23, -1):
        if v >> i & 1:
            v ^= GENERATOR << (i - 24)
    return v


def with_crc(data11):
    return bytes(data11) + crc24(data11).to_bytes(3, "big")


def keeps(filter, msg):
    if filter & DF17 and msg[0] >> 3 != 17:
        return False
    if filter & CRC and crc24(msg[:11]) ^ int.from_bytes(msg[11:14], "big"):
        return False
    return True


def beast_marks(B):
    """Positions of the marks of one stream: the last byte of every odd maximal 0x1A run that a byte follows."""
    marks, N, a = [], len(B), 0
    while a < N:
        if B[a] != 0x1A:
            a += 1
            continue
        b = a
        while b < N and B[b] == 0x1A:
            b += 1
        if b < N and (b - a) % 2 == 1:
            marks.append(b - 1)
        a = b
    return marks


def read_beast(B, m):
    """(state, end, payload) of the mark at m: state in unknown / cut / incomplete / complete."""
    N, kind = len(B), B[m + 1]
    if kind not in LENGTHS:
        return "unknown", m + 2, b""
    need, p, out = 7 + LENGTHS[kind], m + 2, bytearray()
    while len(out) < need:
        if p >= N:
            return "incomplete", p, b""
        v = B[p]
        if v != 0x1A:
            out.append(v)
            p += 1
        elif p + 1 >= N:
            return "incomplete", p, b""
        elif B[p + 1] == 0x1A:
            out.append(0x1A)
            p += 2
        else:
            return "cut", p, b""
    return "complete", p, bytes(out)


def parse_beast_stream(B):
    """One stream -> (events, consumed, counters); an event is (pos, t, s, kind, msg) per complete '3' frame."""
    events, c = [], dict(n_marks=0, n_cut=0, n_unknown=0, n_other=0)
    incomplete, last_end = None, 0
    for m in beast_marks(B):
        c["n_marks"] += 1
        state, end, out = read_beast(B, m)
        if state == "unknown":
            c["n_unknown"] += 1
        elif state == "cut":
            c["n_cut"] += 1
        elif state == "incomplete":
            assert incomplete is None
            incomplete = m
        else:
            assert m >= last_end, "complete frames never overlap"
            last_end = end
            if B[m + 1] == 0x33:
                events.append((m, int.from_bytes(out[:6], "big"), out[6], 0x33, out[7:]))
            else:
                c["n_other"] += 1
    N = len(B)
    if incomplete is not None:
        assert incomplete == beast_marks(B)[-1] and N - incomplete <= 43
        consumed = incomplete
    else:
        k = 0
        while k < N and B[N - 1 - k] == 0x1A and N - 1 - k >= last_end:
            k += 1
        consumed = N - k % 2
    return events, consumed, c


def parse_avr_stream(B):
    events, c = [], dict(n_marks=0, n_cut=0, n_unknown=0, n_other=0)
    N, consumed = len(B), len(B)
    for p in range(N):
        if B[p] not in b"*@":
            continue
        c["n_marks"] += 1
        star, h = B[p] == 0x2A, 0
        while h < 41 and p + 1 + h < N and B[p + 1 + h] in HEX:
            h += 1
        after = p + 1 + h
        if h < 41 and after < N and B[after] == 0x3B:
            digits = B[p + 1:after].decode()
            if h == (28 if star else 40):
                t = 0 if star else int(digits[:12], 16)
                events.append((p, t, 0, B[p], bytes.fromhex(digits[-28:])))
            elif h in ((4, 14) if star else (16, 26)):
                c["n_other"] += 1
            else:
                c["n_cut"] += 1
        elif after == N and h <= (28 if star else 40):
            consumed = p
        else:
            c["n_cut"] += 1
    return events, consumed, c


def parse(stream, stream_ends=None, fmt=BEAST, filter=0, tick_bias=0, max_frames=0, sample_type=I8, levels=False):
    """The whole definition -> dict(frames, rx, levels, counts, consumed, header)."""
    stream = bytes(stream)
    ends = [len(stream)] if stream_ends is None else [int(e) for e in stream_ends]
    assert ends[-1] == len(stream) and ends == sorted(ends)
    cap = len(stream) // 23 if not max_frames else min(int(max_frames), len(stream) // 23)
    header = dict.fromkeys(HEADER_FIELDS, 0)
    rows, counts, consumed, start = [], [], [], 0
    for r, end in enumerate(ends):
        events, used, c = (parse_beast_stream if fmt == BEAST else parse_avr_stream)(stream[start:end])
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
    header["flags"] = TRUNCATED if len(rows) > cap else 0
    rows = rows[:cap]
    fr, rx = np.zeros(len(rows), dtype=FRAME_DTYPE), np.zeros(len(rows), dtype=RX_DTYPE)
    lv = np.zeros(len(rows), dtype=LEVEL_DTYPE) if levels else None
    for i, (r, pos, t, s, kind, msg) in enumerate(rows):
        fr[i] = (((t - tick_bias) % (1 << 48)) // 6, np.frombuffer(msg, dtype=np.uint8), 0, 0xFF)
        rx[i] = (t, pos, s, kind, r)
        if levels and s:
            lv[i]["signal_sum"], lv[i]["flags"] = smallest_sum_for(s, sample_type), 1
    return dict(frames=fr, rx=rx, levels=lv, counts=np.array(counts, dtype=np.uint64),
                consumed=np.array(consumed, dtype=np.uint64), header=header)


def same(got, want, what=""):
    """A library result (air_rs_amd.WireIn) against the model's, byte for byte."""
    assert {k: int(got.header[k]) for k in HEADER_FIELDS} == want["header"], (what, got.header, want["header"])
    assert got.counts.tolist() == want["counts"].tolist(), (what, got.counts, want["counts"])
    assert got.consumed.tolist() == want["consumed"].tolist(), (what, got.consumed, want["consumed"])
    assert got.frames.tobytes() == want["frames"].tobytes(), (what, "frames")
    assert got.rx.tobytes() == want["rx"].tobytes(), (what, "rx", got.rx[:4], want["rx"][:4])
    assert (got.levels is None) == (want["levels"] is None), what
    if got.levels is not None:
        assert got.levels.tobytes() == want["levels"].tobytes(), (what, "levels")


def parse_chunked(stream, chunk, parser, fmt=BEAST):
    """One stream fed `chunk` new bytes at a time with the unparsed tail carried by consumed -> (frames with absolute
    positions as [(pos, t, s, msg)], the longest tail).  parser(bytes) -> an object with .frames, .rx, .consumed or the
    model's dict."""
    out, tail, origin, longest, fed = [], b"", 0, 0, 0
    while True:
        piece = tail + stream[fed:fed + chunk]
        fed += chunk
        res = parser(piece)
        res = res if isinstance(res, dict) else res._asdict()
        for f, x in zip(res["frames"], res["rx"]):
            out.append((origin + int(x["pos"]), int(x["ticks"]), int(x["signal"]), f["bytes"].tobytes()))
        used = int(res["consumed"][0])
        tail, origin = piece[used:], origin + used
        longest = max(longest, len(tail))
        if fed >= len(stream):
            break
    return out, longest


def whole(stream, parser):
    res = parser(stream)
    res = res if isinstance(res, dict) else res._asdict()
    return [(int(x["pos"]), int(x["ticks"]), int(x["signal"]), f["bytes"].tobytes()) for f, x in zip(res["frames"], res["rx"])]


ALPHABET = [0x1A] * 3 + [0x33] * 2 + [0x31, 0x32, 0x34, 0x00, None]


def random_stream(rng, n):
    """n bytes over {1A x3, '3' x2, '1', '2', '4', 00, random}."""
    picks = rng.integers(0, len(ALPHABET), size=n)
    rand = rng.integers(0, 256, size=n)
    return bytes(int(rand[i]) if ALPHABET[p] is None else ALPHABET[p] for i, p in enumerate(picks))
