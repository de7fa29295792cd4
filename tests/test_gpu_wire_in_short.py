"""Wire input with ADSB_WIRE_IN_SHORT on the device: the device parser against the CPU mirror (and the model of
tests/wire_in_short_model.py) on the CPU tier's streams, at stream sizes that straddle the bytes per workgroup span of
adsb_debug_wire_in_geometry, with a short frame cut by the span's edge at every one of its byte positions."""
import ctypes as C

import numpy as np
import pytest

import air_rs_amd as A
from air_rs_amd import _lib
from tests import modes_model as MM
from tests import wire_in_model as M
from tests import wire_in_short_model as S
from tests import wire_model as W
from tests.test_gpu_correlate import _dev

pytestmark = pytest.mark.gpu
FILTERS = {"crc": M.CRC, "df17": M.DF17, "short": S.SHORT}


def _B():
    b, s = C.c_uint32(), C.c_uint32()
    assert _lib.load().adsb_debug_wire_in_geometry(C.byref(b), C.byref(s)) == A.ADSB_OK
    return b.value


@pytest.fixture(scope="module")
def ctx(gpu):
    with A.AdsbDemod(max_samples=1 << 16, max_out=1024) as d:
        yield d


def _check(d, stream, ends=None, **kw):
    """device == mirror == model; returns the device's result"""
    got = d.wire_in_of(stream, ends, **kw)
    mk = dict(kw)
    names = mk.pop("filter", ())
    bits = sum(FILTERS[f] for f in ([names] if isinstance(names, str) else names))
    fmt = mk.pop("format", W.BEAST)
    mk.pop("sample_type", None)
    want = S.parse(stream, ends, fmt=fmt, filter=bits, **mk)
    M.same(got, want, (len(stream), ends, kw, "device"))
    M.same(A.host_wire_parse(stream, ends, **kw), want, (len(stream), ends, kw, "mirror"))
    return got


def test_mixed_streams_of_the_cpu_tier(ctx):
    for seed in range(3):
        rng = np.random.default_rng(500 + seed)
        stream, ends = S.mixed_beast(rng, 120, one_in=3 + seed)
        got = _check(ctx, stream, filter="short", levels=True, tick_bias=seed * 1000)
        assert set(got.rx["kind"].tolist()) == {ord("2"), ord("3")} and got.header["n_other"] > 5
        _check(ctx, stream, [int(ends[40]), int(ends[80]) - 5, len(stream)], filter="short")
        for names in ("crc", ["short", "crc"], ["short", "df17"], ()):
            _check(ctx, stream, filter=names)
        text, tends = S.mixed_avr(np.random.default_rng(600 + seed), 150)
        for fmt in (W.AVR, W.AVR_MLAT):
            _check(ctx, text, format=fmt, filter="short", tick_bias=77)
            _check(ctx, text, [int(tends[30]) - 3, int(tends[30]) - 3, len(text)], format=fmt, filter=["short", "crc"])
            _check(ctx, text, format=fmt)


def test_filters_and_capacity(ctx):
    msgs = [MM.all_call(0x4840D6), MM.all_call(0x4840D6, iid=5), MM.reply(4, 0x4840D6, field=0x0AB0), W.KNOWN,
            MM.reply(20, 0x4840D6)] * 60
    parts = [S.beast_frame(b"2" if len(m) == 7 else b"3", 100 * k, k & 0xFF, m) for k, m in enumerate(msgs)]
    stream, half = b"".join(parts), len(b"".join(parts[:150]))
    assert len(_check(ctx, stream, filter="short", levels=True).frames) == 300
    assert len(_check(ctx, stream, filter=["short", "crc"]).frames) == 120
    assert len(_check(ctx, stream, filter=["short", "df17"]).frames) == 60
    for cap in (1, 255, 256, 257, 299, 300, 301):
        got = _check(ctx, stream, [half, len(stream)], filter="short", max_frames=cap, levels=True)
        assert got.header["total_found"] == 300 and got.header["flags"] == (A.ADSB_FLAG_TRUNCATED if cap < 300 else 0)
    # the densest list there is: 16-byte frames only, max_frames = 0 holds them all
    b = _B()
    one = MM.all_call(0x123456)
    n = 2 * b // 16 + 3
    beast = b"".join(S.beast_frame(b"2", 0x40 + (k & 0x3F), 0, one) for k in range(n))
    star = S.avr_line(one, eol=b"") * n
    assert len(beast) == len(star) == 16 * n
    for stream, fmt in ((beast, W.BEAST), (star, W.AVR)):
        got = _check(ctx, stream, format=fmt, filter="short")
        assert len(got.frames) == n and got.header["flags"] == 0
        dev = _dev(np.frombuffer(stream, dtype=np.uint8))
        two = ctx.wire_in_of((dev.data_ptr(), len(stream)), format=fmt, filter="short")            # device memory, run to run
        assert all(x.tobytes() == y.tobytes() for x, y in zip(got[:2], two[:2]))
        del dev


def test_a_short_frame_cut_by_the_span_edge_at_every_byte(ctx):
    b = _B()
    msg = MM.reply(5, 0x1A2B3C, field=0x1A1A & 0x1FFF)
    rng = np.random.default_rng(5)
    shapes = ((S.beast_frame(b"2", 0x1A0000001A1A, 0x1A, msg), W.BEAST), (S.avr_line(msg, t=0xABCDEF012345), W.AVR),
              (S.avr_line(msg), W.AVR))
    for frame, fmt in shapes:
        for g in range(b - len(frame) - 1, b + 2):                  # the frame starts g bytes in: every byte of it meets the edge
            garbage = bytes(int(x) if x not in (0x1A, 0x2A, 0x40) else 0 for x in rng.integers(0, 256, size=g))
            got = _check(ctx, garbage + frame + garbage[:40], format=fmt, filter="short", levels=True)
            assert got.rx["pos"].tolist() == [g] and got.frames["bytes"][0].tobytes() == msg + bytes(7)
            got = _check(ctx, garbage + frame[:-1], format=fmt, filter="short")                 # and one byte short of it
            short_by_one = fmt == W.AVR and frame.endswith(b";\n")    # (an AVR line is whole at its ';')
            assert len(got.frames) == (1 if short_by_one else 0)
        for size in (b - 1, b, b + 1, 2 * b + 1):                   # streams of frames whose sizes straddle the span
            reps = size // len(frame) + 1
            stream = (frame * reps)[:size]
            got = _check(ctx, stream, format=fmt, filter="short")
            assert len(got.frames) >= size // len(frame) - 1
            _check(ctx, stream, format=fmt)                                                      # the bit clear: n_other
