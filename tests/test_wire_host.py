"""Wire output, CPU tier: the CPU mirror (adsb_host_wire_encode) against literal known answers and, byte for byte, against
the independent model (tests/wire_model.py), whose parser must give every stream's frames back."""
import numpy as np
import pytest

from tests import levels_cases as K
from tests import wire_model as W


def _check(lib, frames, levels=None, sample_type=W.I8, tick_bias=0, formats=W.FORMATS):
    """mirror == model for stream and ends, and parse(stream) == the list; returns the Beast stream"""
    first = None
    for fmt in formats:
        got, ends = lib.host_wire_encode(frames, levels, format=fmt, sample_type=sample_type, tick_bias=tick_bias)
        want, want_ends = W.encode(fmt, frames, levels, sample_type, tick_bias)
        assert got == want, (fmt, got[:64].hex(), want[:64].hex())
        assert ends.dtype == np.uint32 and ends.tolist() == want_ends.tolist(), fmt
        assert W.parse(fmt, got) == W.expected_parse(fmt, frames, levels, sample_type, tick_bias), fmt
        assert b"".join(W.split(got, ends)) == got and (len(frames) == 0 or ends[-1] == len(got))
        first = got if first is None else first
    return first


def test_known_answers(lib):
    fr = W.frame_list([0], [W.KNOWN])
    beast, ends = lib.host_wire_encode(fr)
    assert beast == bytes.fromhex("1A 33 00 00 00 00 00 00 00 8D 48 40 D6 20 2C C3 71 C3 2C E0 57 60 98") and list(ends) == [23]
    avr, ends = lib.host_wire_encode(fr, format="avr")
    assert avr == b"*8D4840D6202CC371C32CE0576098;\n" and list(ends) == [31]
    fr = W.frame_list([1], [W.KNOWN])
    mlat, ends = lib.host_wire_encode(fr, format="avr_mlat", tick_bias=768)
    assert mlat == b"@000000000306" + b"8D4840D6202CC371C32CE0576098;\n" and list(ends) == [43]   # 6 x 1 + 768 = 0x306
    beast, _ = lib.host_wire_encode(fr, tick_bias=768)
    assert beast[2:8] == bytes.fromhex("000000000306")
    # the model gives the same literals
    assert W.encode_one(W.BEAST, 0, W.KNOWN) == bytes.fromhex("1A33000000000000008D4840D6202CC371C32CE0576098")
    assert W.encode_one(W.AVR_MLAT, 1, W.KNOWN, tick_bias=768) == mlat


def test_fixture_frames_with_their_levels(lib):
    iq, fr = K.fixture("ref_frames_i8")
    lv = lib.host_frame_levels(iq, fr)
    assert len(fr) == 7
    beast = _check(lib, fr, lv)
    assert {m[1] for m in W.parse(W.BEAST, beast)} == {W.signal_byte(986000, W.I8)} == {130}   # 255 sqrt(8500 / 32768)
    _check(lib, fr)                                        # and without levels: s = 0
    iq, fr = K.fixture("ref_frames_i16")
    _check(lib, fr, lib.host_frame_levels(iq, fr), sample_type=W.I16)


def test_empty_and_single(lib):
    for fmt in W.FORMATS:
        got, ends = lib.host_wire_encode(W.frame_list([], []), format=fmt)
        assert got == b"" and len(ends) == 0
    _check(lib, W.frame_list([5], [W.KNOWN]), W.level_list([12345]))


def test_every_payload_byte_escaped(lib):
    fr, lv = W.all_1a_frame()
    beast = _check(lib, fr, lv)
    assert len(beast) == 44 and beast == b"\x1a\x33" + b"\x1a" * 42
    assert W.parse(W.BEAST, beast) == [(0x1A1A1A1A1A1A, 0x1A, W.ALL_1A)]
    # between two plain frames: 23 + 44 + 23
    three = np.concatenate([W.plain_frame(1), fr, W.plain_frame(2)])
    got, ends = lib.host_wire_encode(three, np.concatenate([W.level_list([0]), lv, W.level_list([0])]))
    assert list(ends) == [23, 67, 90]


def test_timestamp_wrap_and_bias(lib):
    wrap = (1 << 48) // 6                                   # 6 x wrap = 2^48 - 4
    offs = [wrap - 1, wrap, wrap + 1, wrap + 2, (1 << 64) - 1, 1 << 63, (1 << 64) // 6, (1 << 64) // 6 + 1]
    fr = W.frame_list(offs, [W.KNOWN] * len(offs))
    beast = _check(lib, fr)
    ts = [m[0] for m in W.parse(W.BEAST, beast)]
    assert ts[:4] == [(1 << 48) - 10, (1 << 48) - 4, 2, 8] and all(0 <= t < 1 << 48 for t in ts)
    _check(lib, fr, tick_bias=(1 << 48) - 1)
    one = W.frame_list([0, 1], [W.KNOWN] * 2)
    got, _ = lib.host_wire_encode(one, format="avr_mlat", tick_bias=(1 << 48) - 1)
    assert got[:13] == b"@FFFFFFFFFFFF" and got[43:56] == b"@000000000005"


@pytest.mark.parametrize("st", [W.I8, W.I16], ids=["i8", "i16"])
def test_signal_byte_at_every_rounding_boundary(lib, st):
    sums, want = [0, 1, 116 * W.FULL_SCALE[st], 116 * W.FULL_SCALE[st] - 1, 116 * W.FULL_SCALE[st] + 1, (1 << 64) - 1], \
                 [0, 1, 255, 255, 255, 255]
    for s in range(1, 256):
        lo = W.smallest_sum_for(s, st)
        sums += [lo, lo - 1]
        want += [s, s - 1]
    assert [W.signal_byte_by_definition(x, st) for x in sums] == want   # the model, pinned by the definition's boundaries
    assert [W.signal_byte(x, st) for x in sums] == want                 # and its closed form
    rng = np.random.default_rng(6)
    for x in (rng.random(300) ** 3 * 117 * W.FULL_SCALE[st]).astype(np.uint64):
        assert W.signal_byte(x, st) == W.signal_byte_by_definition(x, st), x
    # half-up rounding: 255 sqrt(sum / (116 FS)) is within a hair above s - 1/2 at the boundary
    for s in (2, 77, 255):
        lo = W.smallest_sum_for(s, st)
        assert 255 * (lo / (116 * W.FULL_SCALE[st])) ** 0.5 >= s - 0.5 > 255 * ((lo - 1) / (116 * W.FULL_SCALE[st])) ** 0.5
    fr = W.frame_list(range(len(sums)), [W.KNOWN] * len(sums))
    beast = _check(lib, fr, W.level_list(sums), sample_type=st, formats=(W.BEAST,))
    assert [m[1] for m in W.parse(W.BEAST, beast)] == want


def test_invalid_level_record_and_no_signal(lib):
    fr = W.frame_list([10, 20], [W.KNOWN] * 2)
    lv = W.level_list([500000, 500000])
    lv["flags"][1] = 0
    beast = _check(lib, fr, lv)
    assert [m[1] for m in W.parse(W.BEAST, beast)] == [W.signal_byte(500000, W.I8), 0]
    lv["flags"][1] = 0xFFFE                                 # every bit but ADSB_LEVEL_VALID
    _check(lib, fr, lv)


def test_random_lists(lib):
    fr = W.random_frames(700, seed=1)
    lv = W.random_levels(700, seed=2)
    beast = _check(lib, fr, lv)
    assert len({len(m) for m in W.split(beast, W.encode(W.BEAST, fr, lv)[1])}) > 6   # many different lengths
    _check(lib, fr, W.random_levels(700, seed=3, sample_type=W.I16), sample_type=W.I16, tick_bias=123456789)


def test_cap_short_by_one_byte_at_every_boundary(lib):
    fr = np.concatenate([W.plain_frame(1), W.all_1a_frame()[0], W.random_frames(6, seed=4)])
    lv = W.random_levels(len(fr), seed=5)
    for fmt in W.FORMATS:
        full, ends = W.encode(fmt, fr, lv)
        for cap in sorted({0, 1, len(full) + 1} | {int(e) + d for e in ends for d in (-1, 0, 1)}):
            got, got_ends = lib.host_wire_encode(fr, lv, format=fmt, cap=cap)
            assert got == full[:W.whole_frames(ends, cap)], (fmt, cap)
            assert got_ends.tolist() == ends.tolist(), (fmt, cap)        # every end, and so the full length
