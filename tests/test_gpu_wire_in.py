"""Wire input on the device (adsb_wire_in_of, adsb_fetch_wire_in, adsb_wire_in_device): every output is compared byte for
byte with the independent sequential model (tests/wire_in_model.py) at every size and position at which the kernels take
another path -- B bytes per workgroup span and S threads in the one-workgroup scans, from adsb_debug_wire_in_geometry --
with lists in host and in device memory, through the encoder and back, and end to end from a launch into correlate."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import air_rs_amd as A
from air_rs_amd import _lib
from tests import correlate_model as CM
from tests import wire_in_model as M
from tests import wire_model as W
from tests.test_gpu_correlate import _dev, _read_device, _shifted_channels

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAME = W.encode_one(W.BEAST, 7, W.KNOWN)


def _geometry():
    b, s = C.c_uint32(), C.c_uint32()
    assert _lib.load().adsb_debug_wire_in_geometry(C.byref(b), C.byref(s)) == A.ADSB_OK
    return b.value, s.value


@pytest.fixture(scope="module")
def ctx(gpu):
    with A.AdsbDemod(max_samples=1 << 16, max_out=1024) as d:
        yield d


def _check(d, stream, ends=None, want=None, **kw):
    """wire_in_of == model (and == the CPU mirror); returns the device's result"""
    got = d.wire_in_of(stream, ends, **kw)
    mk = dict(kw)
    names = mk.pop("filter", ())
    bits = sum({"crc": M.CRC, "df17": M.DF17}[f] for f in ([names] if isinstance(names, str) else names))
    want = M.parse(stream, ends, fmt=mk.pop("format", W.BEAST), filter=bits, **mk) if want is None else want
    M.same(got, want, (len(stream), ends, kw))
    return got


def _device_arrays(d, n_streams, levels):
    """the result read where wire_in_device() says it is, after the stream has drained"""
    got = d.fetch_wire_in()                                                                      # waits
    f, x, lv, cnt, used, h = d.wire_in_device()
    n = len(got.frames)
    hdr = _read_device(h, np.dtype("<u8"), 8)
    assert hdr.tolist() == [int(got.header[k]) for k in M.HEADER_FIELDS]
    assert (lv is not None) == levels
    return A.WireIn(_read_device(f, W.FRAME_DTYPE, n), _read_device(x, M.RX_DTYPE, n),
                    _read_device(lv, W.LEVEL_DTYPE, n) if levels else None, _read_device(cnt, np.dtype("<u8"), n_streams),
                    _read_device(used, np.dtype("<u8"), n_streams), got.header)


# ---- 1: round trips at every list size at which a kernel takes another path ------------------------------------------------
def test_round_trip_sizes(ctx):
    b, s = _geometry()
    long_n = (s * b + b) // 23 + 50                    # its stream is longer than S x B + B bytes: the carry loops run twice
    for n in (0, 1, 255, 256, 257, 515, long_n):
        fr, lv = W.random_frames(n, seed=200 + n % 1000, one_in=8), W.random_levels(n, seed=300 + n % 1000)
        stream, ends = W.encode(W.BEAST, fr, lv)
        assert n != long_n or len(stream) > s * b + b
        want = M.parse(stream, levels=True)
        assert want["frames"]["bytes"].tobytes() == fr["bytes"].tobytes() and want["header"]["n_marks"] == n
        got = _check(ctx, stream, want=want, levels=True)
        M.same(_device_arrays(ctx, 1, True), want, (n, "device arrays"))
        assert got.rx["pos"].tolist() == ([0] + ends[:-1].tolist())[:n]
        M.same(A.host_wire_parse(stream, levels=True), want, (n, "mirror"))
        dev = _dev(np.frombuffer(stream, dtype=np.uint8)) if n else None
        if n:
            M.same(ctx.wire_in_of((dev.data_ptr(), len(stream)), levels=True), want, (n, "device memory"))
            two = ctx.wire_in_of((dev.data_ptr(), len(stream)), levels=True)                       # run to run: the same bytes
            assert all(x.tobytes() == y.tobytes() for x, y in zip(got[:5], two[:5]))
            if n < 1000:                                                                          # an input at every alignment
                for lead in (1, 2, 3):
                    shifted = _dev(np.frombuffer(b"\x1a" * lead + stream, dtype=np.uint8))
                    M.same(ctx.wire_in_of((shifted.data_ptr() + lead, len(stream)), levels=True), want, (n, "lead", lead))
                    del shifted
        again, again_ends = ctx.wire_of(got.frames, got.levels)                                   # wire_of(wire_in_of(x)) == x
        assert again == stream and again_ends.tolist() == ends.tolist()
        del dev


# ---- 2: one frame at every position across a span boundary -----------------------------------------------------------------
def test_one_frame_across_the_span_boundary(ctx):
    b, _ = _geometry()
    fr, lv = W.all_1a_frame()
    long_frame = W.encode(W.BEAST, fr, lv)[0]                                                     # 44 bytes: the whole halo
    rng = np.random.default_rng(5)
    for g in range(b - 45, b + 2):
        garbage = bytes(int(x) if x != 0x1A else 0 for x in rng.integers(0, 256, size=g))
        for frame in (FRAME, long_frame):
            got = _check(ctx, garbage + frame)
            assert got.rx["pos"].tolist() == [g] and got.consumed.tolist() == [g + len(frame)]
        got = _check(ctx, garbage + long_frame[:-1])                                              # and one byte short of it
        assert len(got.frames) == 0 and got.consumed.tolist() == [g]


# ---- 3: runs that cross spans, spans that are wholly 0x1A ------------------------------------------------------------------
def test_runs_in_front_of_a_frame(ctx):
    b, _ = _geometry()
    for k in (1, 2, 3, b - 1, b, b + 1, 2 * b, 2 * b + 1, 3 * b + 2):
        for lead in (b"", b"\x00" * 7):
            got = _check(ctx, lead + b"\x1a" * k + FRAME[1:])
            assert len(got.frames) == k % 2 == got.header["n_marks"]
            got = _check(ctx, lead + b"\x1a" * k)                                                 # the run reaches the end
            assert got.consumed.tolist() == [len(lead) + k - k % 2] and got.header["n_marks"] == 0
        # the run starts in an earlier stream: only the part inside the frame's own stream counts
        got = _check(ctx, b"\x1a" * k + FRAME[1:], [k // 2, k + 22])
        assert len(got.frames) == (k - k // 2) % 2 and got.counts.tolist() == [0, (k - k // 2) % 2]
        assert got.consumed.tolist() == [k // 2 - (k // 2) % 2, k - k // 2 + 22]


# ---- 4, 5: hostile density, random garbage ----------------------------------------------------------------------------------
def test_the_densest_hostile_stream(ctx):
    b, _ = _geometry()
    stream = (b"\x1a\x33" * (b + 1))[:2 * b + 1]
    got = _check(ctx, stream)
    assert len(got.frames) == 0 and got.header["n_marks"] == b and got.header["n_cut"] == b - 1
    assert got.consumed.tolist() == [2 * b - 2]              # every mark is cut by the next; the last one is incomplete


def test_random_garbage(ctx):
    b, _ = _geometry()
    rng = np.random.default_rng(77)
    stream = M.random_stream(rng, 4 * b + 13)
    got = _check(ctx, stream)
    assert got.header["n_cut"] > 100 and got.header["n_other"] > 20 and got.header["n_unknown"] > 100
    cuts = sorted(int(x) for x in rng.integers(1, len(stream), size=9))
    _check(ctx, stream, cuts + [len(stream)])                                                     # and as ten streams
    avr = bytes(b"*@;0aF\n\x1a"[int(x)] for x in rng.integers(0, 8, size=2 * b + 5))
    _check(ctx, avr, format=W.AVR)
    _check(ctx, avr, cuts[:4] + [len(avr)], format=W.AVR_MLAT)


# ---- 6: truncated tails, chunks ---------------------------------------------------------------------------------------------
def test_truncated_tails_and_chunks(ctx):
    fr = W.random_frames(300, seed=31, one_in=4)
    stream, ends = W.encode(W.BEAST, fr, W.random_levels(300, seed=32))
    last = int(ends[-2])
    for c in (last + 1, last + 2, last + 9, len(stream) - 1, len(stream)):
        got = _check(ctx, stream[:c])
        assert got.consumed.tolist() == [last if c < len(stream) else c] and len(got.frames) == 299 + (c == len(stream))
    whole = M.whole(stream, M.parse)
    out, longest = M.parse_chunked(stream, 1000, lambda piece: ctx.wire_in_of(piece))
    assert out == whole and len(out) == 300 and 0 < longest <= 43


# ---- 7: filters and max_frames ----------------------------------------------------------------------------------------------
def test_filters_and_max_frames(ctx):
    good = [M.with_crc(bytes([0x8D, 0x48, 0x40, 0xD6, k & 0xFF, k >> 8, 0xC3, 0x71, 0xC3, 0x2C, 0xE0])) for k in range(400)]
    msgs = []
    for k, g in enumerate(good):
        msgs.append(g if k % 3 else bytes([g[0], g[1] ^ 0x04]) + g[2:])                           # one bit flipped
        if k % 5 == 0:
            msgs.append(M.with_crc(bytes([0x5D]) + g[1:11]))                                      # DF 11, valid CRC
    fr = W.frame_list(range(100, 100 + len(msgs)), msgs)
    stream, _ = W.encode(W.BEAST, fr)
    assert len(_check(ctx, stream).frames) == len(msgs)
    got = _check(ctx, stream, filter="crc")
    assert got.header["n_rejected"] == 134 and len(got.frames) == len(msgs) - 134
    got = _check(ctx, stream, filter="df17")
    assert got.header["n_rejected"] == 80
    got = _check(ctx, stream, filter=["crc", "df17"])
    assert got.frames["bytes"].tobytes() == b"".join(g for k, g in enumerate(good) if k % 3)
    cuts = [len(stream) // 3, len(stream) // 3, len(stream)]
    full = _check(ctx, stream, cuts, levels=True)
    for cap in (1, 255, 256, 257, len(msgs) - 1, len(msgs), len(msgs) + 1):
        got = _check(ctx, stream, cuts, max_frames=cap, levels=True)
        assert got.header["total_found"] == len(msgs) and len(got.frames) == min(cap, len(msgs))
        assert got.header["flags"] == (A.ADSB_FLAG_TRUNCATED if cap < len(msgs) else 0)
        assert got.counts.tolist() == np.diff(np.minimum(np.cumsum([0] + full.counts.tolist()), cap)).tolist()


# ---- 8: streams laid end to end ---------------------------------------------------------------------------------------------
def test_three_streams(ctx):
    b, _ = _geometry()
    fr = W.random_frames(400, seed=41, one_in=5)
    body, _ = W.encode(W.BEAST, fr)
    s0 = body + b"\x00\x1a"                                       # ends in 1A ...
    s1 = FRAME[1:] + body                                         # ... and the next begins with 33: no mark spans the boundary
    streams = [s0, b"", s1, b"\x1a", FRAME[:20]]
    got = _check(ctx, b"".join(streams), np.cumsum([len(x) for x in streams]), levels=True)
    assert got.counts.tolist() == [400, 0, 400, 0, 0] and len(b"".join(streams)) > 4 * b
    assert got.consumed.tolist() == [len(s0) - 1, 0, len(s1), 0, 0]
    assert got.rx["receiver"].tolist() == [0] * 400 + [2] * 400 and got.rx["pos"][400] == 22
    M.same(_device_arrays(ctx, 5, True), M.parse(b"".join(streams), np.cumsum([len(x) for x in streams]), levels=True), "device")
    # 256 streams, most of them empty or a byte long
    ends = np.minimum(np.arange(1, 257) * 3, len(body))
    ends[-1] = len(body)
    _check(ctx, body, ends)


# ---- 9: AVR -----------------------------------------------------------------------------------------------------------------
def test_avr(ctx):
    fr = W.random_frames(257, seed=51)
    for fmt, bias in ((W.AVR, 0), (W.AVR_MLAT, 12345)):
        text, ends = W.encode(fmt, fr, tick_bias=bias)
        got = _check(ctx, text, format=fmt, tick_bias=bias, levels=True)
        assert got.frames["bytes"].tobytes() == fr["bytes"].tobytes() and got.rx["pos"].tolist() == [0] + ends[:-1].tolist()
        if fmt == W.AVR_MLAT:
            assert got.frames["offset"].tolist() == fr["offset"].tolist()
        assert ctx.wire_of(got.frames, format=fmt, tick_bias=bias)[0] == text
        _check(ctx, text.lower().replace(b"\n", b"\r\n")[:-7], format=fmt)
        _check(ctx, text, [31 * 4 + 5, 31 * 4 + 5, len(text)], format=fmt)


# ---- 10: end to end ---------------------------------------------------------------------------------------------------------
def test_from_a_launch_through_the_wire_into_correlate(gpu):
    n, delays = 50_000, [0, 1234, 4321]
    dev = _dev(_shifted_channels(n, delays))
    with A.AdsbDemod(max_samples=n, max_out=1 << 14, max_channels=3, host_staging=False) as d:
        L = _lib.load()
        assert L.adsb_fetch_wire_in(d.handle, None, None, None, 0, None, None, None, 0, None) == A.ADSB_E_STATE
        assert L.adsb_wire_in_device(d.handle, None, None, None, None, None, None) == A.ADSB_E_STATE
        d.demod_device_async(dev.data_ptr(), n, n_channels=3, channel_stride=n)
        frames, counts, total, flags = d.fetch()
        lv = d.levels()
        assert flags == 0 and min(counts) > 30
        cuts = np.cumsum([0] + list(counts))
        parts = [d.wire_of(frames[a:b], lv[a:b])[0] for a, b in zip(cuts, cuts[1:])]               # per receiver, to Beast
        stream, ends = b"".join(parts), np.cumsum([len(p) for p in parts])
        got = d.wire_in_of(stream, ends, levels=True)
        M.same(got, M.parse(stream, ends, levels=True), "launch")
        plain = frames.copy()
        plain["status"], plain["fixed_bit"] = 0, 0xFF
        assert got.frames.tobytes() == plain.tobytes() and got.counts.tolist() == [int(c) for c in counts]
        assert [W.signal_byte(x["signal_sum"], W.I8) if x["flags"] & 1 else 0 for x in got.levels] == got.rx["signal"].tolist()
        assert got.rx["signal"].tolist() == [W.level_signal(x, W.I8) for x in lv]
        want = d.correlate_of(plain, counts, 0, delays, got.levels)
        CM.same(want, CM.correlate(plain, counts, 0, delays, got.levels), "model")
        f, _, lvd, _, _, _ = d.wire_in_device()                                                   # the parsed list where it lies
        again = d.correlate_of((f, len(frames)), got.counts, 0, delays, lvd)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(again, want)) and (want[0]["n_receivers"] == 3).sum() > 30
        assert (want[0]["best_receiver"] != 0xFFFF).sum() > 30
    del dev


# ---- 11: untouched paths; the argument checks that need a device -----------------------------------------------------------
def test_other_results_stay_as_they_are(gpu):
    cfg = A.synth_default(seed=5, slot_len=800)
    n = 40_000
    dev = _dev(np.concatenate([A.synth_fill_host(cfg, A.ADSB_SAMPLE_I8, c, 0, n) for c in range(2)]))
    with A.AdsbDemod(max_samples=n, max_out=1 << 12, max_channels=2, host_staging=False) as d:
        d.demod_device_async(dev.data_ptr(), n, n_channels=2, channel_stride=n)
        frames, counts, total, flags = d.fetch()
        lv = d.levels()
        wire = d.wire("beast", signal=True)
        corr = d.correlate(50, levels=True)
        assert len(frames) > 40
        got = d.wire_in_of(wire[0], levels=True)
        assert len(got.frames) == len(frames)
        d.wire_in_of(W.encode(W.AVR, W.random_frames(3000, seed=1))[0], format="avr")            # grows the buffers
        again, counts2, total2, flags2 = d.fetch()
        assert again.tobytes() == frames.tobytes() and list(counts2) == list(counts) and (total2, flags2) == (total, flags)
        assert d.levels().tobytes() == lv.tobytes()
        back = d.fetch_wire()
        assert back[0] == wire[0] and back[1].tolist() == wire[1].tolist()
        assert all(x.tobytes() == y.tobytes() for x, y in zip(d.fetch_correlated(), corr))
    del dev


def test_argument_checks(ctx):
    L, h = _lib.load(), ctx.handle
    want = ctx.wire_in_of(FRAME * 3, [23, 69], levels=True)
    ok = _lib.AdsbWireInCfg(0, 0, 0, 0, 0, 0)

    def call(cfg=ok, data=FRAME, n=23, ends=(23,), R=None):
        e = None if ends is None else np.array(ends, dtype=np.uint64)
        return L.adsb_wire_in_of(h, None if cfg is None else C.byref(cfg), data, n, None if e is None else e.ctypes.data,
                                 (len(e) if e is not None else 1) if R is None else R)

    assert L.adsb_wire_in_of(None, C.byref(ok), FRAME, 23, np.array([23], dtype=np.uint64).ctypes.data, 1) == A.ADSB_E_ARG
    assert call(cfg=None) == A.ADSB_E_ARG and call(data=None) == A.ADSB_E_ARG and call(ends=None) == A.ADSB_E_ARG
    assert call(cfg=_lib.AdsbWireInCfg(3, 0, 0, 0, 0, 0)) == A.ADSB_E_ARG
    assert call(cfg=_lib.AdsbWireInCfg(0, 0, 1 << 48, 0, 0, 0)) == A.ADSB_E_ARG
    assert call(cfg=_lib.AdsbWireInCfg(0, 0, 0, 0, 2, 1)) == A.ADSB_E_ARG
    assert call(R=0) == A.ADSB_E_ARG and call(ends=[0] * 256 + [23]) == A.ADSB_E_ARG
    assert call(ends=(10, 5, 23)) == A.ADSB_E_ARG and call(ends=(10, 22)) == A.ADSB_E_ARG
    assert call(n=1 << 32, ends=(1 << 32,)) == A.ADSB_E_CAPACITY
    M.same(ctx.fetch_wire_in(), M.parse(FRAME * 3, [23, 69], levels=True), "rejected calls leave the result")
    # short capacities: the totals whatever they are, the first entries
    fr, hdr, n = np.zeros(2, dtype=W.FRAME_DTYPE), _lib.AdsbWireInHeader(), C.c_size_t()
    cnt = np.zeros(1, dtype=np.uint64)
    assert L.adsb_fetch_wire_in(h, fr.ctypes.data, None, None, 2, C.byref(n), cnt.ctypes.data, None, 1, C.byref(hdr)) == A.ADSB_OK
    assert (n.value, hdr.n_frames, hdr.total_found) == (2, 3, 3) and fr.tobytes() == want.frames[:2].tobytes() and cnt[0] == 1
    assert L.adsb_fetch_wire_in(h, None, None, None, 0, None, None, None, 3, None) == A.ADSB_E_ARG   # more streams than parsed
    assert call(data=None, n=0, ends=(0,)) == A.ADSB_OK
    assert L.adsb_fetch_wire_in(h, fr.ctypes.data, None, None, 2, C.byref(n), cnt.ctypes.data, None, 1, C.byref(hdr)) == A.ADSB_OK
    assert (n.value, hdr.n_frames, hdr.n_marks, cnt[0]) == (0, 0, 0, 0)
    lv = np.zeros(1, dtype=W.LEVEL_DTYPE)
    assert L.adsb_fetch_wire_in(h, None, None, lv.ctypes.data, 1, None, None, None, 0, None) == A.ADSB_E_STATE  # no levels asked
    empty = ctx.wire_in_of(b"", [0, 0])
    assert len(empty.frames) == 0 and empty.consumed.tolist() == [0, 0] and empty.levels is None


# ---- 12: the replay tool ----------------------------------------------------------------------------------------------------
def test_replay_tool_reads_what_it_wrote(gpu, tmp_path):
    cfg = A.synth_default(seed=11, slot_len=900)
    iq = A.synth_fill_host(cfg, A.ADSB_SAMPLE_I8, 0, 0, 200_000)
    capture, beast, avr = tmp_path / "capture.u8", tmp_path / "frames.beast", tmp_path / "frames.avr"
    (iq.astype(np.int16) + 128).astype(np.uint8).tofile(capture)
    tool = [sys.executable, os.path.join(ROOT, "tools", "replay.py")]
    first = subprocess.run(tool + [str(capture), "--beast", str(beast), "--avr", str(avr)], capture_output=True, text=True,
                           cwd=ROOT, timeout=120)
    assert first.returncode == 0, first.stderr
    assert first.stdout.count("\n") > 30 and beast.stat().st_size > 23 * 30
    for flag, path in (("--beast-in", beast), ("--avr-in", avr)):
        second = subprocess.run(tool + [str(path), flag], capture_output=True, text=True, cwd=ROOT, timeout=120)
        assert second.returncode == 0, second.stderr
        assert second.stdout == first.stdout, flag
