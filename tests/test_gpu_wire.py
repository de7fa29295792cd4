"""Wire output on the device (adsb_wire_device_async, adsb_fetch_wire, adsb_wire_device, adsb_wire_of): stream and ends
are compared byte for byte with the independent model (tests/wire_model.py) at every list size at which the three
kernels take another path, with the 44-byte frame at the edges of a workgroup's span, with lists in host and in device
memory, and through launches of every shape."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import air_rs_amd as A
from air_rs_amd import _lib
from tests import levels_cases as K
from tests import wire_model as W

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _geometry():
    b, t = C.c_uint32(), C.c_uint32()
    assert _lib.load().adsb_debug_wire_geometry(C.byref(b), C.byref(t)) == A.ADSB_OK
    return b.value, t.value


def _dev(arr):
    import torch
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).reshape(-1)).cuda()


def _same(got, want, what):
    (gs, ge), (ws, we) = got, want
    assert ge.dtype == np.uint32 and ge.tolist() == we.tolist(), (what, len(ge), len(we))
    if gs != ws:
        k = next(i for i in range(min(len(gs), len(ws))) if gs[i] != ws[i]) if len(gs) == len(ws) else -1
        raise AssertionError((what, len(gs), len(ws), k, gs[max(k - 8, 0):k + 8].hex(), ws[max(k - 8, 0):k + 8].hex()))


@pytest.fixture(scope="module")
def ctx(gpu):
    with A.AdsbDemod(max_samples=1 << 16, max_out=1024) as d:
        yield d


@pytest.fixture(scope="module")
def big_list():
    """One random list above (threads of the totals scan x frames per workgroup), its levels, and the model's Beast
    stream: the smaller sizes are prefixes of it."""
    b, t = _geometry()
    n = b * t + 1
    fr, lv = W.random_frames(n, seed=21), W.random_levels(n, seed=22)
    stream, ends = W.encode(W.BEAST, fr, lv)
    return fr, lv, stream, ends


# ---- 1: every size at which a kernel takes another path ----------------------------------------------------------------
def test_wire_of_sizes(ctx, big_list):
    b, t = _geometry()
    fr, lv, stream, ends = big_list
    assert len({int(e) % 4 for e in ends[b - 1::b]}) == 4             # workgroup spans start at every alignment mod 4
    for n in (0, 1, b - 1, b, b + 1, 2 * b + 3, b * t + 1):
        want = (stream[:int(ends[n - 1]) if n else 0], ends[:n])
        _same(ctx.wire_of(fr[:n], lv[:n]), want, n)
    n = 2 * b + 3
    for fmt in (W.AVR, W.AVR_MLAT):
        _same(ctx.wire_of(fr[:n], lv[:n], format=fmt, tick_bias=77), W.encode(fmt, fr[:n], tick_bias=77), (fmt, n))
    _same(ctx.wire_of(fr[:n]), W.encode(W.BEAST, fr[:n]), "no levels")
    _same(ctx.wire_of(fr[:n], lv[:n], tick_bias=(1 << 48) - 1), W.encode(W.BEAST, fr[:n], lv[:n], tick_bias=(1 << 48) - 1), "bias")
    # run to run: the same bytes
    assert ctx.wire_of(fr[:n], lv[:n])[0] == ctx.wire_of(fr[:n], lv[:n])[0] == stream[:int(ends[n - 1])]


# ---- 2: the 44-byte frame at the edges of a workgroup's span -----------------------------------------------------------
def _hot_list(n, hot_at):
    fr = W.frame_list([1] * n, [W.KNOWN] * n)               # 23 bytes each: no 0x1A in the timestamp or the frame
    lv = W.level_list([0] * n)
    hot_f, hot_l = W.all_1a_frame()
    for k in hot_at:
        fr[k], lv[k] = hot_f[0], hot_l[0]
    return fr, lv


@pytest.mark.parametrize("fmt", W.FORMATS)
def test_wire_of_all_1a_frame_at_span_edges(ctx, fmt):
    b, _ = _geometry()
    n = 2 * b + 5
    for hot_at in ([b], [b - 1], [b - 1, b], [0, n - 1], [b + 7], list(range(b - 2, b + 3)), [2 * b - 1, 2 * b]):
        fr, lv = _hot_list(n, hot_at)
        want = W.encode(fmt, fr, lv)
        if fmt == W.BEAST:
            sizes = [len(m) for m in W.split(*want)]
            assert all(size == (44 if k in hot_at else 23) for k, size in enumerate(sizes))
        _same(ctx.wire_of(fr, lv, format=fmt), want, (fmt, hot_at))
    # the parser gets the hot frame back
    fr, lv = _hot_list(3, [1])
    got, ends = ctx.wire_of(fr, lv, format=fmt)
    assert ends.tolist() == W.encode(fmt, fr, lv)[1].tolist()
    assert W.parse(fmt, got) == W.expected_parse(fmt, fr, lv)
    if fmt == W.BEAST:
        assert list(ends) == [23, 67, 90]


# ---- 3: lists in host and in device memory; cap; the edge lists of the CPU tier -----------------------------------------
def test_wire_of_memory_kinds_and_cap(ctx):
    fr, lv = W.random_frames(300, seed=31), W.random_levels(300, seed=32)
    want = W.encode(W.BEAST, fr, lv)
    dfr, dlv = _dev(fr), _dev(lv)
    _same(ctx.wire_of((dfr.data_ptr(), len(fr)), dlv.data_ptr()), want, "device, device")
    _same(ctx.wire_of((dfr.data_ptr(), len(fr)), lv), want, "device, host")
    _same(ctx.wire_of(fr, dlv.data_ptr()), want, "host, device")
    _same(ctx.wire_of(fr, lv), want, "host, host")
    assert ctx.wire_of(fr, lv)[0] == A.host_wire_encode(fr, lv)[0]
    del dfr, dlv
    stream, ends = want
    for cap in (0, 22, 23, int(ends[0]) - 1, int(ends[0]), int(ends[149]) - 1, int(ends[149]) + 1, len(stream) - 1, len(stream)):
        got, got_ends = ctx.wire_of(fr, lv, cap=cap)
        assert got == stream[:W.whole_frames(ends, cap)] and got_ends.tolist() == ends.tolist(), cap
    # i16 full scale, wrap of the timestamp, an invalid level record
    wrap = (1 << 48) // 6
    fr = W.frame_list([wrap - 1, wrap, wrap + 1, (1 << 64) - 1, 5], [W.KNOWN] * 5)
    lv = W.level_list([0, 1, 116 << 31, (1 << 64) - 1, 99999])
    lv["flags"][4] = 0
    with A.AdsbDemod(sample_type=A.ADSB_SAMPLE_I16, max_samples=1 << 16, max_out=64) as d16:
        _same(d16.wire_of(fr, lv), W.encode(W.BEAST, fr, lv, W.I16), "i16")
        table = [W.smallest_sum_for(s, W.I16) - d for s in range(1, 256) for d in (0, 1)]
        tf = W.frame_list(range(len(table)), [W.KNOWN] * len(table))
        _same(d16.wire_of(tf, W.level_list(table)), W.encode(W.BEAST, tf, W.level_list(table), W.I16), "i16 table")
    table = [W.smallest_sum_for(s, W.I8) - d for s in range(1, 256) for d in (0, 1)]
    tf = W.frame_list(range(len(table)), [W.KNOWN] * len(table))
    got = ctx.wire_of(tf, W.level_list(table))
    _same(got, W.encode(W.BEAST, tf, W.level_list(table)), "i8 table")
    assert [m[1] for m in W.parse(W.BEAST, got[0])] == [s - d for s in range(1, 256) for d in (0, 1)]


# ---- 4: through a launch ------------------------------------------------------------------------------------------------
def _model_of_launch(d, fmt, st, signal, tick_bias=0):
    frames, counts, total, flags = d.fetch()
    assert flags == 0 and len(frames) == total
    lv = d.levels() if signal else None
    return frames, counts, W.encode(fmt, frames, lv, st, tick_bias)


@pytest.mark.parametrize("nch", [1, 5])
def test_through_a_launch(gpu, nch):
    cfg = A.synth_default(seed=3, slot_len=800)
    n = 70_000 + 8
    buf = np.concatenate([A.synth_fill_host(cfg, A.ADSB_SAMPLE_I8, c, 0, n) for c in range(nch)])
    dev = _dev(buf)
    with A.AdsbDemod(max_samples=n, max_out=1 << 12, max_channels=nch, host_staging=False) as d:
        L = _lib.load()
        cnt, cnt2, ptr = C.c_size_t(), C.c_size_t(), C.c_void_p()
        wcfg = _lib.AdsbWireCfg(A.ADSB_WIRE_BEAST, 1, 0)
        assert L.adsb_wire_device_async(d.handle, C.byref(wcfg)) == A.ADSB_E_STATE            # before any launch
        assert L.adsb_wire_device(d.handle, C.byref(ptr), None, None) == A.ADSB_E_STATE
        d.demod_device_async(dev.data_ptr(), n, n_channels=nch, channel_stride=n)
        assert L.adsb_fetch_wire(d.handle, None, 0, C.byref(cnt), None, 0, C.byref(cnt2)) == A.ADSB_E_STATE   # nothing enqueued
        assert L.adsb_wire_device_async(d.handle, C.byref(_lib.AdsbWireCfg(3, 0, 0))) == A.ADSB_E_ARG
        assert L.adsb_wire_device_async(d.handle, C.byref(_lib.AdsbWireCfg(0, 0, 1 << 48))) == A.ADSB_E_ARG
        got = d.wire("beast", signal=True)                   # the levels are enqueued by the call
        frames, counts, want = _model_of_launch(d, W.BEAST, W.I8, True)
        assert len(frames) > 60 * nch and min(counts) > 10
        _same(got, want, "beast + signal")
        assert {m[1] for m in W.parse(W.BEAST, got[0])} - {0} and W.parse(W.BEAST, got[0]) == \
            W.expected_parse(W.BEAST, frames, d.levels())
        # per_channel_counts cut the stream per receiver without parsing it
        pos = 0
        for c in range(nch):
            a = int(got[1][pos - 1]) if pos else 0
            part = got[0][a:int(got[1][pos + counts[c] - 1])]
            assert [m[2] for m in W.parse(W.BEAST, part)] == [f["bytes"].tobytes() for f in frames[pos:pos + counts[c]]]
            pos += counts[c]
        # another format on the same launch replaces the first
        _same(d.wire("avr_mlat", tick_bias=240 * 6), W.encode(W.AVR_MLAT, frames, tick_bias=1440), "avr_mlat")
        _same(d.fetch_wire(), W.encode(W.AVR_MLAT, frames, tick_bias=1440), "fetched again")
        _same(d.wire("avr"), W.encode(W.AVR, frames), "avr")
        _same(d.wire("beast", signal=False), W.encode(W.BEAST, frames), "beast, no signal")
        # short capacities: whole frames only
        stream, ends = want
        d.wire_async("beast", signal=True)
        for cap in (0, int(ends[3]) - 1, int(ends[3]), len(stream) - 1):
            part, few = d.fetch_wire(cap=cap, max_ends=5)
            assert part == stream[:W.whole_frames(ends, cap)] and few.tolist() == ends[:5].tolist(), cap
        b, e, h = d.wire_device()
        assert b and e and h
        # a stream base: the timestamps run on
        d.set_stream_base(1 << 40)
        d.demod_device_async(dev.data_ptr(), n, n_channels=nch, channel_stride=n)
        assert L.adsb_fetch_wire(d.handle, None, 0, C.byref(cnt), None, 0, C.byref(cnt2)) == A.ADSB_E_STATE   # the last launch's
        got = d.wire("beast", signal=True, tick_bias=5)
        based, _, want = _model_of_launch(d, W.BEAST, W.I8, True, tick_bias=5)
        assert (based["offset"] == frames["offset"] + np.uint64(1 << 40)).all()
        _same(got, want, "stream base")
        assert [m[0] for m in W.parse(W.BEAST, got[0])] == [(6 * (int(o) + (1 << 40)) + 5) % (1 << 48) for o in frames["offset"]]
    del dev


def test_through_a_launch_cs16_and_one_dispatch_path(gpu):
    cfg = A.synth_default(seed=8, slot_len=700)
    cfg.amp_shift = 6
    n = 50_000
    iq = A.synth_fill_host(cfg, A.ADSB_SAMPLE_I16, 0, 0, n)
    with A.AdsbDemod(sample_type=A.ADSB_SAMPLE_I16, max_samples=n, max_out=1 << 12) as d:
        frames, flags = d.demod(iq)                           # adsb_demod: the staged copy of the buffer
        assert flags == 0 and len(frames) > 30
        got = d.wire("beast", signal=True)
        _same(got, W.encode(W.BEAST, frames, d.levels(), W.I16), "cs16")
        assert got[0] == A.host_wire_encode(frames, A.host_frame_levels(iq, frames), sample_type=A.ADSB_SAMPLE_I16)[0]
        _same(d.wire("avr_mlat"), W.encode(W.AVR_MLAT, frames), "cs16 avr_mlat")
    iq, want = K.fixture("ref_frames_i8")
    with A.AdsbDemod(max_samples=len(iq), max_out=64) as d:
        frames, flags = d.demod(iq)
        assert frames.tobytes() == want.tobytes()
        _same(d.wire("beast", signal=True), W.encode(W.BEAST, frames, A.host_frame_levels(iq, frames)), "fixture")
        _same(d.wire("avr"), W.encode(W.AVR, frames), "fixture avr")


# ---- 5: the list is rebuilt after a slot-pool overflow ---------------------------------------------------------------
def test_slot_pool_repair(gpu):
    cfg = A.synth_default(seed=19, slot_len=600)
    iq = A.synth_fill_host(cfg, A.ADSB_SAMPLE_I8, 0, 0, 120_000).copy()
    iq[40_000:60_000] = (3, 4)            # constant: one frame per offset, tiles far over their 32 slots
    with A.AdsbDemod(max_samples=len(iq), max_out=1 << 15) as d:
        d.pool_limit(True)
        dev = _dev(iq)
        d.demod_device_async(dev.data_ptr(), len(iq))
        d.wire_async("beast", signal=True)                    # enqueued on the list with holes
        got = d.fetch_wire()                                  # the wait rebuilds the list, the levels and the stream
        d.pool_limit(False)
        frames, _, total, flags = d.fetch()
        assert flags == 0 and len(frames) == total > 15_000
        _same(got, W.encode(W.BEAST, frames, d.levels()), "rebuilt")
        d.demod_device_async(dev.data_ptr(), len(iq))         # and without the knob: the same stream
        _same(d.wire("beast", signal=True), got, "plain")
        del dev


# ---- 6: tools/replay.py --beast / --avr ------------------------------------------------------------------------------
def test_replay_beast_and_avr(gpu, tmp_path):
    iq, want = K.fixture("ref_frames_i16")
    path, beast, avr = tmp_path / "capture.c16", tmp_path / "out.beast", tmp_path / "out.avr"
    iq.astype("<i2").tofile(path)
    tool = os.path.join(ROOT, "tools", "replay.py")
    r = subprocess.run([sys.executable, tool, str(path), "--chunk", "3000", "--carry", "--tail", "--summary",
                        "--beast", str(beast), "--avr", str(avr), "--mlat", "--tick-bias", "11"],
                       capture_output=True, text=True, timeout=300, check=True)
    counted = int(re.search(r"(\d+) packets", r.stderr).group(1))
    msgs = W.parse(W.BEAST, beast.read_bytes())
    assert len(msgs) == counted == len(want) == 7
    lv = A.host_frame_levels(iq, want)
    assert msgs == W.expected_parse(W.BEAST, want, lv, W.I16, tick_bias=11)
    assert beast.read_bytes() == W.encode(W.BEAST, want, lv, W.I16, tick_bias=11)[0]
    assert avr.read_bytes() == W.encode(W.AVR_MLAT, want, tick_bias=11)[0]
    assert W.parse(W.AVR_MLAT, avr.read_bytes()) == W.expected_parse(W.AVR_MLAT, want, tick_bias=11)
