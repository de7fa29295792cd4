"""Wire input with ADSB_WIRE_IN_SHORT, CPU tier: adsb_host_wire_parse against the model with short-frame emission
(tests/wire_in_short_model.py) on streams that mix '1' / '2' / '3' in Beast and all six AVR shapes, with doubled 0x1A
bytes inside short frames, each filter bit, the capacity rule, chunked parsing, and -- with the bit clear -- the
behaviour from before the bit: short frames counted in n_other."""
import numpy as np
import pytest

from tests import modes_model as MM
from tests import wire_in_model as M
from tests import wire_in_short_model as S
from tests import wire_model as W

FILTERS = {"crc": M.CRC, "df17": M.DF17, "short": S.SHORT}


def _check(lib, stream, ends=None, **kw):
    got = lib.host_wire_parse(stream, ends, **kw)
    mk = dict(kw)
    names = mk.pop("filter", ())
    bits = sum(FILTERS[f] for f in ([names] if isinstance(names, str) else names))
    M.same(got, S.parse(stream, ends, fmt=mk.pop("format", W.BEAST), filter=bits, **mk), (stream[:40].hex(), ends, kw))
    return got


def test_the_bit_and_its_names(lib):
    assert lib.ADSB_WIRE_IN_SHORT == lib.WIRE_IN_SHORT == 4
    one = S.beast_frame(b"2", 600, 9, MM.all_call(0x4840D6))
    by_name, by_bit = lib.host_wire_parse(one, filter="short"), lib.host_wire_parse(one, filter=lib.WIRE_IN_SHORT)
    assert by_name.frames.tobytes() == by_bit.frames.tobytes() and len(by_bit.frames) == 1


def test_one_short_frame_in_each_shape(lib):
    msg = MM.all_call(0x1A1A1A, iid=0)                              # the address doubles on the wire
    assert msg.count(b"\x1a") >= 3
    beast = S.beast_frame(b"2", 0x1A0000001A06, 0x1A, msg)
    assert len(beast) == 16 + 3 + msg.count(b"\x1a")
    got = _check(lib, beast, filter="short", levels=True)
    assert got.frames["bytes"][0].tobytes() == msg + bytes(7) and got.frames["offset"].tolist() == [0x1A0000001A06 // 6]
    assert (got.frames["status"], got.frames["fixed_bit"]) == (0, 0xFF) and got.rx["kind"].tolist() == [ord("2")]
    assert got.rx["signal"].tolist() == [0x1A] and got.levels["flags"].tolist() == [1]
    assert got.levels["signal_sum"].tolist() == [W.smallest_sum_for(0x1A, W.I8)]
    assert got.header["n_other"] == 0 and got.consumed.tolist() == [len(beast)]
    star, at = S.avr_line(msg), S.avr_line(msg, t=0xABCDEF012345)
    assert len(star) == 17 and len(at) == 29
    for fmt in (W.AVR, W.AVR_MLAT):
        got = _check(lib, star + at.lower(), format=fmt, filter="short", tick_bias=5, levels=True)
        assert got.rx["kind"].tolist() == [ord("*"), ord("@")] and got.rx["ticks"].tolist() == [0, 0xABCDEF012345]
        assert got.frames["bytes"].tobytes() == (msg + bytes(7)) * 2 and not got.levels.tobytes().strip(b"\0")
        assert got.frames["offset"].tolist() == [((0 - 5) % (1 << 48)) // 6, (0xABCDEF012345 - 5) // 6]


@pytest.mark.parametrize("seed", range(6))
def test_mixed_beast_streams(lib, seed):
    rng = np.random.default_rng(500 + seed)
    stream, ends = S.mixed_beast(rng, 120, one_in=3 + seed)
    assert stream.count(b"\x1a\x1a") > 20
    got = _check(lib, stream, filter="short", levels=True, tick_bias=seed * 1000)
    kinds = set(got.rx["kind"].tolist())
    assert kinds == {ord("2"), ord("3")} and got.header["n_other"] > 5 and got.header["n_cut"] == 0
    assert got.header["n_marks"] == 120 == got.header["n_other"] + len(got.frames)
    short = got.rx["kind"] == ord("2")
    assert (got.frames["bytes"][short][:, 7:] == 0).all()
    # three streams laid end to end, one of them cut inside a short frame
    cuts = [int(ends[40]), int(ends[80]) - 5, len(stream)]
    _check(lib, stream, cuts, filter="short")
    # with the bit clear: what the parser did before the bit existed
    old = _check(lib, stream, levels=True, tick_bias=seed * 1000)
    assert set(old.rx["kind"].tolist()) == {ord("3")} and old.header["n_other"] == 120 - len(old.frames)
    assert old.frames.tobytes() == got.frames[~short].tobytes() and old.consumed.tolist() == got.consumed.tolist()
    M.same(old, M.parse(stream, levels=True, tick_bias=seed * 1000), "the old model itself")


@pytest.mark.parametrize("seed", range(3))
def test_mixed_avr_streams(lib, seed):
    rng = np.random.default_rng(600 + seed)
    text, ends = S.mixed_avr(rng, 150)
    for fmt in (W.AVR, W.AVR_MLAT):
        got = _check(lib, text, format=fmt, filter="short", tick_bias=77)
        sizes = [int((row != 0).any()) for row in got.frames["bytes"][:, 7:]]
        assert got.header["n_other"] > 20 and got.header["n_marks"] == 150 and 0 in sizes and 1 in sizes
        assert {ord("*"), ord("@")} == set(got.rx["kind"].tolist())
        _check(lib, text, [int(ends[30]) - 3, int(ends[30]) - 3, len(text)], format=fmt, filter="short")
        old = _check(lib, text, format=fmt, tick_bias=77)
        assert old.header["n_other"] == 150 - len(old.frames) and len(old.frames) < len(got.frames)
    # neighbours of the short shapes are cut, not short
    junk = b"*" + b"0" * 13 + b";*" + b"0" * 15 + b";@" + b"0" * 25 + b";@" + b"0" * 27 + b";*" + b"0" * 14 + b"\n;"
    got = _check(lib, junk, format=W.AVR, filter="short")
    assert len(got.frames) == 0 and got.header["n_cut"] == 5


def test_truncated_at_every_byte_of_a_short_frame(lib):
    msg = MM.reply(4, 0x1A2B1A, field=0x1A)
    for tail in (S.beast_frame(b"2", 0x1A1A, 0x1A, msg), S.avr_line(msg, t=7), S.avr_line(msg)):
        fmt = W.BEAST if tail[0] == 0x1A else W.AVR
        head = S.beast_frame(b"3", 5, 6, W.KNOWN) if fmt == W.BEAST else S.avr_line(W.KNOWN)
        for c in range(len(tail) + 1):
            got = _check(lib, head + tail[:c], format=fmt, filter="short")
            whole = c == len(tail) or (fmt == W.AVR and c == len(tail) - 1)
            assert len(got.frames) == 1 + whole
            assert got.consumed.tolist() == [len(head) + (c if whole or c == 0 else 0)], c


def test_filters_are_literal(lib):
    good11 = MM.all_call(0x4840D6)                                 # a short frame with a zero syndrome
    iid11 = MM.all_call(0x4840D6, iid=5)                           # an interrogator's reply: a non-zero syndrome
    ap4 = MM.reply(4, 0x4840D6, field=0x0AB0)                      # address/parity: never a zero syndrome
    short17 = bytes([17 << 3]) + good11[1:]                        # DF17 in its first byte, but a short frame
    long17, long20 = W.KNOWN, MM.reply(20, 0x4840D6)
    msgs = [good11, iid11, ap4, short17, long17, long20, MM.overlay(short17[:4], 0)]
    stream = b"".join(S.beast_frame(b"2" if len(m) == 7 else b"3", 100 * k, k, m) for k, m in enumerate(msgs))
    assert len(_check(lib, stream, filter="short").frames) == 7
    got = _check(lib, stream, filter=["short", "crc"])
    assert got.frames["bytes"][:, :7].tobytes() == good11 + long17[:7] + msgs[6] and got.header["n_rejected"] == 4
    got = _check(lib, stream, filter=["short", "df17"])
    assert got.frames["bytes"].tobytes() == long17 and got.header["n_rejected"] == 6       # every short frame rejected
    got = _check(lib, stream, filter=["short", "crc", "df17"])
    assert got.frames["bytes"].tobytes() == long17 and got.header["n_rejected"] == 6
    assert got.consumed.tolist() == [len(stream)] and got.header["n_marks"] == 7 and got.header["n_other"] == 0
    # rejected short frames are still frames for the framing: a stream cut inside its last one carries it
    assert _check(lib, stream[:-2], filter=["short", "df17"]).consumed.tolist() == [len(stream) - 16]
    text = b"".join(S.avr_line(m, t=k) for k, m in enumerate(msgs))
    got = _check(lib, text, format=W.AVR, filter=["short", "crc"])
    assert got.header["n_rejected"] == 4 and len(got.frames) == 3
    # without the bit the filters see long frames only
    got = _check(lib, stream, filter="crc")
    assert len(got.frames) == 1 and got.header["n_other"] == 5 and got.header["n_rejected"] == 1


def test_max_frames_zero_never_truncates_the_shortest_frames(lib):
    msg = MM.all_call(0x123456)
    assert b"\x1a" not in msg
    for n in (1, 2, 33):
        beast = b"".join(S.beast_frame(b"2", 0x40 + k, 0, msg) for k in range(n))       # (no byte is 0x1A: nothing doubles)
        star = b"".join(S.avr_line(msg, eol=b"") for _ in range(n))
        assert len(beast) == len(star) == 16 * n
        for stream, fmt in ((beast, W.BEAST), (star, W.AVR)):
            got = _check(lib, stream, format=fmt, filter="short")
            assert len(got.frames) == n == got.header["total_found"] and got.header["flags"] == 0
            got = _check(lib, stream, format=fmt, filter="short", max_frames=n + 5)
            assert len(got.frames) == n and got.header["flags"] == 0
            if n > 1:
                got = _check(lib, stream, format=fmt, filter="short", max_frames=n - 1, levels=True)
                assert len(got.frames) == n - 1 and got.header["flags"] == M.TRUNCATED and got.header["total_found"] == n


@pytest.mark.parametrize("chunk", [1, 7, 16, 17, 44])
def test_chunked_parsing_is_parsing_whole(lib, chunk):
    rng = np.random.default_rng(700)
    beast, _ = S.mixed_beast(rng, 60, one_in=4)
    text, _ = S.mixed_avr(rng, 60)
    garbage = M.random_stream(rng, 900)
    for stream, fmt in ((beast, W.BEAST), (text, W.AVR), (garbage, W.BEAST)):
        for bits in (S.SHORT, 0):
            parser = lambda piece: lib.host_wire_parse(piece, format=fmt, filter=bits)
            ref = M.whole(stream, lambda b: S.parse(b, fmt=fmt, filter=bits))
            assert M.whole(stream, parser) == ref
            out, longest = M.parse_chunked(stream, chunk, parser)
            assert out == ref and longest <= 43, (fmt, bits)
        assert len(M.whole(stream, lambda b: S.parse(b, fmt=fmt, filter=S.SHORT))) > len(ref) or stream is garbage
