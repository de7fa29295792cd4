"""Wire input, CPU tier: the CPU mirror (adsb_host_wire_parse) byte for byte against the independent sequential model
(tests/wire_in_model.py), on round trips through the encoder's model, hand-made framings, truncated and chunked
streams, the filters, several streams laid end to end, and AVR text."""
import ctypes as C

import numpy as np
import pytest

from air_rs_amd import _lib as L
from tests import levels_cases as K
from tests import wire_in_model as M
from tests import wire_model as W

T48 = 1 << 48


def _check(lib, stream, ends=None, **kw):
    """mirror == model; returns the mirror's result"""
    got = lib.host_wire_parse(stream, ends, **kw)
    names = kw.pop("filter", ())
    bits = sum({"crc": M.CRC, "df17": M.DF17}[f] for f in ([names] if isinstance(names, str) else names))
    M.same(got, M.parse(stream, ends, fmt=kw.pop("format", W.BEAST), filter=bits, **kw), (stream[:48].hex(), ends, kw))
    return got


def _round_trip(lib, fr, lv=None, sample_type=W.I8, tick_bias=0):
    """parse(encode(x)) == x: bytes, offsets, positions, and the signal bytes back through the encoder"""
    stream, ends = W.encode(W.BEAST, fr, lv, sample_type, tick_bias)
    got = _check(lib, stream, levels=True, sample_type=sample_type, tick_bias=tick_bias)
    n = len(fr)
    assert len(got.frames) == n == got.header["n_frames"] == got.header["n_marks"] and got.counts.tolist() == [n]
    assert got.frames["bytes"].tobytes() == fr["bytes"].tobytes()
    assert got.frames["offset"].tolist() == fr["offset"].tolist()            # (every offset here is below 2^48 / 6)
    assert (got.frames["status"] == 0).all() and (got.frames["fixed_bit"] == 0xFF).all()
    assert got.rx["pos"].tolist() == ([0] + ends[:-1].tolist())[:n] and set(got.rx["kind"].tolist()) <= {0x33}
    assert got.rx["ticks"].tolist() == [W.ticks(o, tick_bias) for o in fr["offset"]]
    assert got.consumed.tolist() == [len(stream)] and got.header["n_cut"] == got.header["n_unknown"] == 0
    again, again_ends = lib.host_wire_encode(got.frames, got.levels, sample_type=sample_type, tick_bias=tick_bias)
    assert again == stream and again_ends.tolist() == ends.tolist()
    return got


def test_round_trip_of_the_fixture_frames_with_their_levels(lib):
    iq, fr = K.fixture("ref_frames_i8")
    lv = lib.host_frame_levels(iq, fr)
    got = _round_trip(lib, fr, lv)
    assert set(got.rx["signal"].tolist()) == {130} and (got.levels["flags"] == 1).all()
    assert got.levels["signal_sum"].tolist() == [W.smallest_sum_for(130, W.I8)] * len(fr)
    iq, fr = K.fixture("ref_frames_i16")
    _round_trip(lib, fr, lib.host_frame_levels(iq, fr), sample_type=W.I16)


@pytest.mark.parametrize("n", [0, 1, 5, 300])
def test_round_trip_one_byte_in_three_escaped(lib, n):
    _round_trip(lib, W.random_frames(n, seed=40 + n, one_in=3), W.random_levels(n, seed=50 + n))


def test_all_1a_frame_alone_and_three_in_a_row(lib):
    fr, lv = W.all_1a_frame()
    got = _round_trip(lib, fr, lv)
    assert got.rx["signal"].tolist() == [0x1A] and got.rx["ticks"].tolist() == [0x1A1A1A1A1A1A]
    three = np.concatenate([fr, fr, fr])
    got = _round_trip(lib, three, np.concatenate([lv, lv, lv]))
    assert got.rx["pos"].tolist() == [0, 44, 88]


def test_timestamps_at_the_top_of_48_bits(lib):
    fr = W.frame_list([0, 1, T48 // 6 - 1, 5], [W.KNOWN, W.ALL_1A, W.KNOWN, W.KNOWN])
    got = _round_trip(lib, fr, tick_bias=T48 - 1)
    assert got.rx["ticks"].tolist()[0] == T48 - 1 and got.frames["offset"].tolist() == [0, 1, T48 // 6 - 1, 5]
    got = _round_trip(lib, fr)
    assert max(got.rx["ticks"].tolist()) == 6 * (T48 // 6 - 1)
    # a timestamp of 2^48 - 1 read with no bias, and with a bias above it
    stream = W.encode_one(W.BEAST, 0, W.KNOWN, tick_bias=T48 - 1)
    assert _check(lib, stream).frames["offset"].tolist() == [(T48 - 1) // 6]
    stream = W.encode_one(W.BEAST, 0, W.KNOWN, tick_bias=5)
    assert _check(lib, stream, tick_bias=T48 - 1).frames["offset"].tolist() == [1]     # (5 - (2^48 - 1)) mod 2^48 = 6


@pytest.mark.parametrize("sample_type", [W.I8, W.I16])
def test_every_signal_byte_through_levels_and_back(lib, sample_type):
    fr = W.random_frames(256, seed=9, one_in=8)
    lv = W.level_list([W.smallest_sum_for(s, sample_type) if s else 0 for s in range(256)])
    lv["flags"][0] = 0
    assert [W.signal_byte(x, sample_type) for x in lv["signal_sum"][1:]] == list(range(1, 256))
    got = _round_trip(lib, fr, lv, sample_type=sample_type)
    assert got.rx["signal"].tolist() == list(range(256))
    assert got.levels.tobytes() == lv.tobytes()


FRAME = W.encode_one(W.BEAST, 7, W.KNOWN)                 # 23 bytes, no 0x1A but the mark


@pytest.mark.parametrize("k", range(1, 7))
def test_a_run_in_front_of_a_frame_marks_iff_odd(lib, k):
    for lead in (b"", b"\x00", b"\x33"):
        got = _check(lib, lead + b"\x1a" * k + FRAME[1:])
        assert len(got.frames) == got.header["n_marks"] == k % 2
        if k % 2:
            assert got.rx["pos"].tolist() == [len(lead) + k - 1]


def _one(t, s, msg, kind=b"3"):
    body = int(t).to_bytes(6, "big") + bytes([s]) + bytes(msg)
    return b"\x1a" + kind + body.replace(b"\x1a", b"\x1a\x1a")


def test_frame_layouts(lib):
    # cut by a mark inside its payload: the second frame is whole
    got = _check(lib, FRAME[:10] + FRAME)
    assert got.header["n_marks"] == 2 and got.header["n_cut"] == 1 and got.rx["pos"].tolist() == [10]
    # a frame whose last byte is 0x1A, then more 0x1A: it ends inside an even run (no mark behind it) ...
    tail_1a = _one(9, 0, W.KNOWN[:13] + b"\x1a")
    got = _check(lib, tail_1a + b"\x1a\x1a" + FRAME[1:])
    assert len(got.frames) == 1 and got.header["n_marks"] == 1
    # ... and inside an odd run: the run's last byte is the next mark
    got = _check(lib, tail_1a + b"\x1a" + FRAME[1:])
    assert got.rx["pos"].tolist() == [0, len(tail_1a)] and got.header["n_marks"] == 2
    # unknown type bytes are counted and nothing is read for them
    got = _check(lib, b"\x1a\x34" + FRAME + b"\x1a\x00" + FRAME + b"\x1a\xff")
    assert got.header["n_unknown"] == 3 and len(got.frames) == 2 and got.consumed.tolist() == [2 * 23 + 6]
    # '1' and '2' frames between '3' frames
    stream = FRAME + _one(1, 2, b"\x1a\x00", b"1") + FRAME + _one(3, 4, b"\x1a" * 7, b"2") + FRAME
    got = _check(lib, stream)
    assert got.header["n_other"] == 2 and len(got.frames) == 3 and got.header["n_marks"] == 5


def test_truncated_at_every_byte_of_the_last_two_frames(lib):
    fr = W.random_frames(4, seed=3, one_in=3)
    fr["bytes"][3][13] = 0x1A                                  # the stream ends in 1A 1A
    stream, ends = W.encode(W.BEAST, fr, W.random_levels(4, seed=4))
    full = M.whole(stream, M.parse)
    for c in range(int(ends[1]), len(stream) + 1):
        got = _check(lib, stream[:c])
        used = int(got.consumed[0])
        assert c - used <= 43 and used >= (int(ends[len(got.frames) - 1]) if len(got.frames) else 0)
        rest = M.whole(stream[used:], lambda b: lib.host_wire_parse(b))
        assert M.whole(stream[:c], lambda b: got) + [(p + used, t, s, m) for p, t, s, m in rest] == full, c


class _Lean:
    """adsb_host_wire_parse of one stream into preallocated arrays (the chunked test makes a million calls)."""

    def __init__(self):
        self.fn = L.load().adsb_host_wire_parse
        self.cfg = L.AdsbWireInCfg(L.ADSB_WIRE_BEAST, 0, 0, 0, 0, 0)
        self.fr, self.rx = np.zeros(16, dtype=W.FRAME_DTYPE), np.zeros(16, dtype=M.RX_DTYPE)
        self.end, self.used, self.n = C.c_uint64(), C.c_uint64(), C.c_size_t()

    def __call__(self, piece):
        self.end.value = len(piece)
        rc = self.fn(C.byref(self.cfg), piece, len(piece), C.byref(self.end), 1, self.fr.ctypes.data, self.rx.ctypes.data,
                     None, 16, C.byref(self.n), None, C.byref(self.used), None)
        assert rc == 0
        n = self.n.value
        return dict(frames=self.fr[:n], rx=self.rx[:n], consumed=[self.used.value])


def test_chunked_parsing_of_3000_random_streams(lib):
    """The caller's next chunk is B[consumed..) + new bytes: the same frames at the same absolute positions as the whole
    parse, in chunks of any size, and never more than 43 bytes carried."""
    rng = np.random.default_rng(2024)
    lean, frames_seen, complete_seen = _Lean(), 0, 0
    for i in range(3000):
        stream = M.random_stream(rng, int(rng.integers(0, 201)))
        want = M.parse(stream)
        M.same(lib.host_wire_parse(stream), want, i)
        ref = [(int(x["pos"]), int(x["ticks"]), int(x["signal"]), f["bytes"].tobytes())
               for f, x in zip(want["frames"], want["rx"])]
        frames_seen += len(ref)
        complete_seen += want["header"]["n_other"]
        for chunk in (1, 2, 3, 7, 44, 45):
            out, longest = M.parse_chunked(stream, chunk, lean)
            assert out == ref and longest <= 43, (i, chunk, stream.hex())
    assert frames_seen > 20 and complete_seen > 500, (frames_seen, complete_seen)


def test_filters(lib):
    good = [M.with_crc(bytes([0x8D, 0x48, 0x40, 0xD6, k, 0x2C, 0xC3, 0x71, 0xC3, 0x2C, 0xE0])) for k in range(6)]
    assert M.with_crc(W.KNOWN[:11]) == W.KNOWN                          # the known frame carries its own CRC
    flipped = [bytes([g[0]] + [g[1] ^ 0x10] + list(g[2:])) for g in good[:2]] + [good[2][:13] + bytes([good[2][13] ^ 1])]
    df11 = M.with_crc(bytes([0x5D]) + good[0][1:11])                       # DF 11 with a valid CRC
    msgs = [good[0], flipped[0], df11, good[1], flipped[1], flipped[2], good[2], W.ALL_1A]
    fr = W.frame_list(range(10, 10 + len(msgs)), msgs)
    stream, ends = W.encode(W.BEAST, fr)
    assert len(_check(lib, stream).frames) == 8
    got = _check(lib, stream, filter="crc")
    assert got.frames["bytes"].tobytes() == b"".join([good[0], df11, good[1], good[2]]) and got.header["n_rejected"] == 4
    got = _check(lib, stream, filter="df17")
    assert len(got.frames) == 6 and got.header["n_rejected"] == 2
    got = _check(lib, stream, filter=["crc", "df17"])
    assert got.frames["bytes"].tobytes() == b"".join(good[:3]) and got.header["n_rejected"] == 5
    assert got.consumed.tolist() == [len(stream)] and got.header["n_marks"] == 8
    # the filters do not touch the framing: the stream cut inside its last frame carries that frame
    assert _check(lib, stream[:-3], filter="crc").consumed.tolist() == [int(ends[-2])]


def test_max_frames_truncates_and_clips_counts(lib):
    fr = W.random_frames(9, seed=8)
    parts = [W.encode(W.BEAST, fr[a:b])[0] for a, b in ((0, 4), (4, 4), (4, 9))]
    stream, ends = b"".join(parts), np.cumsum([len(p) for p in parts])
    for cap, counts in ((0, [4, 0, 5]), (9, [4, 0, 5]), (100, [4, 0, 5]), (8, [4, 0, 4]), (4, [4, 0, 0]), (3, [3, 0, 0]),
                        (1, [1, 0, 0])):
        got = _check(lib, stream, ends, max_frames=cap, levels=True)
        assert got.counts.tolist() == counts and got.header["total_found"] == 9
        assert got.header["flags"] == (M.TRUNCATED if 0 < cap < 9 else 0) and len(got.frames) == sum(counts)
        assert got.frames["bytes"].tobytes() == fr["bytes"][:sum(counts)].tobytes()


def test_no_mark_spans_a_stream_boundary(lib):
    """stream 0 ends in 1A, stream 1 begins with 33...: laid end to end that is a frame's bytes, but not a frame."""
    s0, s1, s2 = FRAME + b"\x00\x1a", FRAME[1:] + FRAME, b"\x1a" + FRAME
    got = _check(lib, s0 + s1 + s2, np.cumsum([len(s0), len(s1), len(s2)]))
    assert got.counts.tolist() == [1, 1, 0] and got.rx["pos"].tolist() == [0, 22]
    assert got.consumed.tolist() == [len(s0) - 1, len(s1), len(s2)] and got.rx["receiver"].tolist() == [0, 1]
    assert got.header["n_marks"] == 2                       # s2: 1A 1A 33 ... holds an even run and no mark


def test_empty_streams(lib):
    got = _check(lib, b"")
    assert len(got.frames) == 0 and got.counts.tolist() == [0] and got.consumed.tolist() == [0]
    got = _check(lib, b"", [0, 0, 0], levels=True)
    assert got.counts.tolist() == [0, 0, 0] and len(got.levels) == 0
    got = _check(lib, FRAME * 2, [0, 23, 23, 46, 46])
    assert got.counts.tolist() == [0, 1, 0, 1, 0] and got.rx["receiver"].tolist() == [1, 3]
    for fmt in (W.AVR, W.AVR_MLAT):
        _check(lib, b"", [0, 0], format=fmt)


def test_avr(lib):
    fr = W.random_frames(40, seed=12)
    star, _ = W.encode(W.AVR, fr)
    at, _ = W.encode(W.AVR_MLAT, fr, tick_bias=77)
    for fmt in (W.AVR, W.AVR_MLAT):                               # both formats read both forms
        got = _check(lib, star, format=fmt)
        assert got.frames["bytes"].tobytes() == fr["bytes"].tobytes() and set(got.rx["kind"].tolist()) == {ord("*")}
        assert (got.rx["ticks"] == 0).all() and (got.frames["offset"] == 0).all() and got.rx["pos"].tolist()[:2] == [0, 31]
        got = _check(lib, at, format=fmt, tick_bias=77, levels=True)
        assert got.frames.tobytes() == M.parse(W.encode(W.BEAST, fr)[0])["frames"].tobytes()
        assert set(got.rx["kind"].tolist()) == {ord("@")} and not got.levels.tobytes().strip(b"\0")
    mixed = star[:31 * 3].lower().replace(b"\n", b"\r\n") + at[:43 * 2] + star[31 * 3:31 * 4]
    got = _check(lib, mixed, format=W.AVR)
    assert got.frames["bytes"].tobytes() == fr["bytes"][[0, 1, 2, 0, 1, 3]].tobytes()
    # garbage lines, short forms, and the 29-digit line
    h = W.KNOWN.hex().encode()
    junk = (b"hello\n*;\n*zz;\n@;\n*" + h[:4] + b";\n*" + h[:14] + b";\n@" + h[:16] + b";\n@" + h[:26] + b";\n*" + h + b"0;\n*" +
            h[:27] + b";\n@" + h + b";\n*" + h + b"\n*" + h + b";*@" + b"0" * 50 + b";\n")
    got = _check(lib, junk, format=W.AVR)
    assert got.header["n_other"] == 4 and len(got.frames) == 1 and got.header["n_cut"] == got.header["n_marks"] - 5
    # an incomplete last line at every cut length
    for line in (star[:31], at[:43]):
        for c in range(len(line) + 1):
            got = _check(lib, star[:62] + line[:c], format=W.AVR)
            whole_line = c >= len(line) - 1
            assert got.consumed.tolist() == [62 + c if whole_line or c == 0 else 62] and len(got.frames) == 2 + whole_line
