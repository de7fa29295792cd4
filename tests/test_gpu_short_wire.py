"""Short Mode S frames out, on the device: adsb_levels_modes_of / adsb_levels_modes_device and the wire output with
ADSB_WIRE_SHORT against the CPU mirror against the independent models, byte for byte, at every list size and alignment
at which the kernels take another path; then the chain samples -> replies scan -> merge -> levels -> wire -> wire input."""
import ctypes as C

import numpy as np
import pytest

import air_rs_amd as A
from air_rs_amd import _lib as L
from tests import levels_modes_model as LM
from tests import modes_model as MM
from tests import replies_cases as RK
from tests import replies_model as RM
from tests import short_wire_cases as K
from tests import wire_model as W

pytestmark = pytest.mark.gpu
DTYPES = {"i8": np.int8, "i16": np.int16}
ST = {"i8": A.ADSB_SAMPLE_I8, "i16": A.ADSB_SAMPLE_I16}
FORMATS = ("beast", "avr", "avr_mlat")


def _dev(arr):
    import torch
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.uint8).reshape(-1)).cuda()


def _hip_runtime():
    """The HIP runtime this process already holds (the one libadsb_hip.so is bound to), for a plain hipMemcpy."""
    for line in open("/proc/self/maps"):
        path = line.split()[-1]
        if "libamdhip64" in path:
            return C.CDLL(path)
    raise RuntimeError("no HIP runtime mapped")


def _records_at(ptr, n):
    hip = _hip_runtime()
    hip.hipMemcpy.argtypes, hip.hipMemcpy.restype = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int], C.c_int
    out = np.zeros(n, dtype=A.LEVEL_DTYPE)
    assert hip.hipMemcpy(out.ctypes.data, ptr, out.nbytes, 2) == 0      # device to host
    return out


def _geometry():
    b, t = C.c_uint32(), C.c_uint32()
    assert L.load().adsb_debug_wire_geometry(C.byref(b), C.byref(t)) == A.ADSB_OK
    return b.value, t.value


def _same(got, want, what):
    (gs, ge), (ws, we) = got, want
    assert ge.dtype == np.uint32 and ge.tolist() == we.tolist(), (what, len(ge), len(we))
    if gs != ws:
        k = next((i for i in range(min(len(gs), len(ws))) if gs[i] != ws[i]), -1)
        raise AssertionError((what, len(gs), len(ws), k, gs[max(k - 8, 0):k + 8].hex(), ws[max(k - 8, 0):k + 8].hex()))


@pytest.fixture(scope="module")
def ctx(gpu):
    made = {st: A.AdsbDemod(sample_type=ST[st], max_samples=1 << 16, max_out=1 << 12, max_channels=4, host_staging=False)
            for st in DTYPES}
    yield made
    for d in made.values():
        d.close()


# ---- levels ------------------------------------------------------------------------------------------------------------
def _device_levels(d, c, ptr, frames=None, **kw):
    frames = c["frames"] if frames is None else frames
    return d.levels_modes_of(ptr, c["n_samples"], frames, c["counts"], c["stride"], c["first"], **kw)


@pytest.mark.parametrize("st", ["i8", "i16"])
@pytest.mark.parametrize("k", range(len(K.LENGTHS) + 1))
def test_levels_device_is_mirror_is_model(ctx, st, k):
    """... with the buffer where it lies and one sample further on, which flips the dword alignment of every i8 window"""
    d, c = ctx[st], K.levels_cases(DTYPES[st])[k]
    mirror = A.host_frame_levels_modes(c["iq"], c["frames"], c["counts"], c["n_samples"], c["stride"], c["first"])
    assert mirror.tobytes() == K.model_levels(c).tobytes()
    bps = c["iq"].itemsize * 2
    shifted, plain = _dev(np.concatenate([c["iq"][:1], c["iq"]])), _dev(c["iq"])
    dframes = _dev(c["frames"])
    garbage = c["frames"].copy()
    garbage["bytes"][K.is_short(garbage), 7:] = 0xFF
    assert plain.data_ptr() % 4 == 0 and shifted.data_ptr() % 4 == 0
    for ptr in (plain.data_ptr(), shifted.data_ptr() + bps):
        got = _device_levels(d, c, ptr)
        assert got.tobytes() == mirror.tobytes(), (c["name"], ptr % 4)
        K.check_levels_expectations(c, got)
        assert _device_levels(d, c, ptr, (dframes.data_ptr(), len(c["frames"]))).tobytes() == mirror.tobytes()
        assert _device_levels(d, c, ptr, garbage).tobytes() == mirror.tobytes()
        assert _device_levels(d, c, ptr, fetch=False) is None            # out = NULL: the records stay on the device
        assert _records_at(d.levels_modes_device(), len(mirror)).tobytes() == mirror.tobytes()
    del shifted, plain, dframes


@pytest.mark.parametrize("st", ["i8", "i16"])
def test_levels_list_sizes(ctx, st):
    """1, 4, 5 frames (one block of four waves, then two) and four times the largest grid plus one: the loop wraps"""
    import torch
    d, c = ctx[st], K.levels_case(DTYPES[st], 367)
    blocks = torch.cuda.get_device_properties(0).multi_processor_count * 8
    n0 = c["counts"][0]
    iq = c["iq"][:367 + K.TAIL]
    dev = _dev(iq)
    many = np.tile(c["frames"][:n0], (4 * blocks + 1 + n0 - 1) // n0)[:4 * blocks + 1]
    want = LM.levels(iq[:367], c["frames"][:n0], first_sample=c["first"])
    want = np.tile(want, len(many) // n0 + 1)[:len(many)]
    for n in (1, 4, 5, 4 * blocks + 1):
        got = d.levels_modes_of(dev.data_ptr(), 367, many[:n], first_sample=c["first"])
        assert got.tobytes() == want[:n].tobytes(), n
    assert A.host_frame_levels_modes(iq[:367], many[:300], first_sample=c["first"]).tobytes() == want[:300].tobytes()
    del dev


def test_levels_arguments_and_what_stays(gpu):
    """the argument rules with a ctx; a ctx that has not called the entry point has no records; the last launch's levels
    and adsb_levels_of's results stay as they are"""
    cfg = A.synth_default(seed=5, slot_len=800)
    n = 40_000
    iq = A.synth_fill_host(cfg, A.ADSB_SAMPLE_I8, 0, 0, n)
    dev = _dev(iq)
    with A.AdsbDemod(max_samples=n, max_out=1 << 12, host_staging=False) as d:
        lib, h = L.load(), d.handle
        p = C.c_void_p(77)
        assert lib.adsb_levels_modes_device(h, C.byref(p)) == A.ADSB_E_STATE and lib.adsb_levels_modes_device(h, None) == A.ADSB_E_ARG
        d.demod_device_async(dev.data_ptr(), n)
        frames = d.fetch()[0]
        lv = d.levels()
        assert len(frames) > 20 and (lv["flags"] == 1).all()
        counts = np.array([len(frames)], dtype=np.uint64)
        out = np.full(len(frames) * 32, 0xEE, dtype=np.uint8)
        ok = [h, dev.data_ptr(), 1, n, n, 0, frames.ctypes.data, counts.ctypes.data, len(frames), out.ctypes.data]
        two = np.array([len(frames), 0], dtype=np.uint64)
        for k, v in ((1, None), (1, dev.data_ptr() + 1), (2, 0), (2, (1 << 20) + 1), (6, None), (7, None), (8, len(frames) - 1)):
            args = list(ok)
            args[k] = v
            assert lib.adsb_levels_modes_of(*args) == A.ADSB_E_ARG, k
        args = list(ok)
        args[2], args[4], args[7] = 2, n - 8, two.ctypes.data             # a stride below n_samples
        assert lib.adsb_levels_modes_of(*args) == A.ADSB_E_ARG
        args = list(ok)
        args[8] = 1 << 32
        assert lib.adsb_levels_modes_of(*args) == A.ADSB_E_CAPACITY
        assert (out == 0xEE).all() and lib.adsb_levels_modes_device(h, C.byref(p)) == A.ADSB_E_STATE
        none = np.zeros(1, dtype=np.uint64)                               # no frames: nothing allocated, no records yet
        assert lib.adsb_levels_modes_of(h, dev.data_ptr(), 1, n, n, 0, None, none.ctypes.data, 0, None) == A.ADSB_OK
        assert lib.adsb_levels_modes_device(h, C.byref(p)) == A.ADSB_E_STATE
        assert lib.adsb_levels_modes_of(*ok) == A.ADSB_OK
        assert out.tobytes() == lv.tobytes()                               # all DF17: adsb_levels_device_async's records
        assert d.levels_of(dev.data_ptr(), n, frames).tobytes() == lv.tobytes()
        assert d.levels_modes_device() not in (0, None, d.levels_device())
        assert d.levels().tobytes() == lv.tobytes() and d.fetch()[0].tobytes() == frames.tobytes()
        kept = d.levels_modes_device()                                    # ... and an earlier call's records stay
        assert lib.adsb_levels_modes_of(h, dev.data_ptr(), 1, n, n, 0, None, none.ctypes.data, 0, None) == A.ADSB_OK
        assert d.levels_modes_device() == kept and _records_at(kept, len(frames)).tobytes() == lv.tobytes()
    del dev


# ---- wire --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big_list():
    b, t = _geometry()
    n = b * t + 1
    fr, lv = K.wire_list(n, seed=21)
    stream, ends = LM.encode("beast", fr, lv)
    return fr, lv, stream, ends


def test_wire_sizes_and_span_residues(ctx, big_list):
    d = ctx["i8"]
    b, t = _geometry()
    fr, lv, stream, ends = big_list
    starts = [0] + [int(e) for e in ends[b - 1::b]]                       # where the workgroups' spans start
    assert {s % 4 for s in starts} == {0, 1, 2, 3}                        # ... at every residue mod 4
    for n in (0, 1, b - 1, b, b + 1, 2 * b + 3, b * t + 1):
        want = (stream[:int(ends[n - 1]) if n else 0], ends[:n])
        _same(d.wire_of(fr[:n], lv[:n], short=True), want, n)
    n = 2 * b + 3
    assert A.host_wire_encode(fr[:n], lv[:n], short=True)[0] == stream[:int(ends[n - 1])]
    for fmt in ("avr", "avr_mlat"):
        want = LM.encode(fmt, fr[:n], None, 0, 77)
        _same(d.wire_of(fr[:n], lv[:n], format=fmt, tick_bias=77, short=True), want, (fmt, n))
    _same(d.wire_of(fr[:n], short=True), LM.encode("beast", fr[:n]), "no levels")
    _same(d.wire_of(fr[:n], lv[:n]), W.encode("beast", fr[:n], lv[:n]), "without the bit: the bytes of before")
    dfr, dlv = _dev(fr[:n]), _dev(lv[:n])
    _same(d.wire_of((dfr.data_ptr(), n), dlv.data_ptr(), short=True), (stream[:int(ends[n - 1])], ends[:n]), "device lists")
    del dfr, dlv


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("mix", ["short", "long", "alternate"])
def test_wire_mixes(ctx, fmt, mix):
    b, _ = _geometry()
    for st in ("i8", "i16"):
        fr, lv = K.wire_list(3 * b + 17, seed=90, mix=mix, sample_type=ST[st])
        _same(ctx[st].wire_of(fr, lv, format=fmt, tick_bias=5, short=True), LM.encode(fmt, fr, lv, ST[st], 5), (fmt, mix, st))


def test_wire_workgroups_of_the_longest_frames(ctx):
    """a workgroup of nothing but 30-byte short frames and one of nothing but 43-byte long ones, their spans starting at
    residue r mod 4 for r = 0..3: the workgroup in front is r frames of 23 bytes and b - r of 22.  (With the bit set a
    long frame cannot be 44 bytes: a first byte of 0x1A is DF3, a short frame; the 44-byte frame without the bit is
    tests/test_gpu_wire.py's.)"""
    d = ctx["i8"]
    b, _ = _geometry()
    assert b % 4 == 0
    hot_f, hot_l, bias = K.hot_short_frame()
    for r in (0, 1, 2, 3):
        n = 3 * b + 2
        fr = W.frame_list([1000] * n, [bytes([0x20, 1, 2, 3, 4, 5, 6]) + bytes(7)] * n)    # 22 bytes: 1A 32, 12 of t, s = 0, 7
        lv = np.zeros(n, dtype=A.LEVEL_DTYPE)
        lv[:r] = hot_l[0]                                                                 # 23 bytes: s = 0x1A
        fr[b:2 * b], lv[b:2 * b] = hot_f[0], hot_l[0]
        fr["bytes"][2 * b:3 * b] = np.frombuffer(bytes([0x8D]) + b"\x1a" * 13, dtype=np.uint8)
        lv[2 * b:3 * b] = W.level_list([W.smallest_sum_for(26, W.I8)])[0]
        want = LM.encode("beast", fr, lv, 0, bias)
        sizes = np.diff(np.concatenate([[0], want[1]])).tolist()
        assert sizes[:b] == [23] * r + [22] * (b - r) and sizes[b:2 * b] == [30] * b and sizes[2 * b:3 * b] == [43] * b
        assert int(want[1][b - 1]) % 4 == int(want[1][2 * b - 1]) % 4 == r
        _same(d.wire_of(fr, lv, tick_bias=bias, short=True), want, r)
        assert A.host_wire_encode(fr, lv, tick_bias=bias, short=True)[0] == want[0]


def test_wire_cap_cuts(ctx):
    d = ctx["i8"]
    fr, lv = K.wire_list(300, seed=60, mix="alternate")
    stream, ends = LM.encode("beast", fr, lv)
    e = [int(x) for x in ends]
    for cap in (0, 15, e[0] - 1, e[0], e[0] + 1, e[1] - 1, e[1], e[2] - 1, e[149] + 7, len(stream) - 1, len(stream)):
        got, got_ends = d.wire_of(fr, lv, cap=cap, short=True)
        assert got == stream[:W.whole_frames(ends, cap)] and got_ends.tolist() == e, cap


def test_wire_of_a_launch_and_the_format_rule(gpu):
    """the demodulator's list is all DF17: wire(short=True) gives the bytes of short=False; the format rule with a ctx"""
    cfg = A.synth_default(seed=5, slot_len=800)
    n = 40_000
    iq = A.synth_fill_host(cfg, A.ADSB_SAMPLE_I8, 0, 0, n)
    with A.AdsbDemod(max_samples=n, max_out=1 << 12) as d:
        frames, flags = d.demod(iq)
        assert len(frames) > 20 and flags == 0
        for fmt in FORMATS:
            plain = d.wire(fmt)
            _same(d.wire(fmt, short=True), plain, fmt)
            _same(plain, W.encode(fmt, frames, d.levels()), fmt)
        lib, h = L.load(), d.handle
        out, nb = np.zeros(64, dtype=np.uint8), C.c_size_t()
        one = W.frame_list([0], [bytes([0x20]) + bytes(13)])
        for fmt in (0, 1, 2, 3, 0xFF, 0x100, 0x101, 0x102, 0x103, 0x200, 0x80000100, 0xFFFFFFFF):
            wc = L.AdsbWireCfg(fmt, 0, 0)
            want = A.ADSB_OK if fmt in (0, 1, 2, 0x100, 0x101, 0x102) else A.ADSB_E_ARG
            assert lib.adsb_wire_of(h, C.byref(wc), one.ctypes.data, None, 1, out.ctypes.data, 64, C.byref(nb), None) == want, hex(fmt)
            assert lib.adsb_wire_device_async(h, C.byref(wc)) == want, hex(fmt)
        stream = np.frombuffer(b"\x1a\x32" + bytes(7) + bytes([0x20]) + bytes(6), dtype=np.uint8)
        ends = np.array([16], dtype=np.uint64)
        for fmt, want in ((0, A.ADSB_OK), (0x100, A.ADSB_E_ARG), (0x102, A.ADSB_E_ARG)):
            ic = L.AdsbWireInCfg(fmt, A.ADSB_WIRE_IN_SHORT, 0, 0, 0, 0)
            assert lib.adsb_wire_in_of(h, C.byref(ic), stream.ctypes.data, 16, ends.ctypes.data, 1) == want, hex(fmt)


def test_replay_sends_the_merged_list_out(gpu, tmp_path):
    """tools/replay.py FILE --replies --beast OUT --levels, and --avr OUT --mlat: the files read back as the merged list"""
    import os
    import subprocess
    import sys
    from tests.test_replies_tool import capture
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    iq, msgs = capture()
    path, beast, avr = tmp_path / "capture.bin", tmp_path / "out.bin", tmp_path / "out.txt"
    (iq.view(np.uint8) ^ 0x80).tofile(path)
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "replay.py"), str(path), "--replies", "--levels", "--beast",
                        str(beast), "--avr", str(avr), "--mlat", "--tick-bias", "12"], capture_output=True, text=True, timeout=120, cwd=root)
    assert r.returncode == 0, r.stderr
    rows = {x.split("\t")[0]: x.split("\t") for x in r.stdout.splitlines()}
    assert [rows[o][1] for o in ("100", "1100", "2100", "3100")] == ["DF11", "DF4", "DF17", "DF20"]
    assert all(-5.3 < float(rows[o][2]) < -5.0 and rows[o][5] == "0" for o in ("100", "1100", "2100", "3100"))
    back = A.host_wire_parse(beast.read_bytes(), filter=A.WIRE_IN_SHORT, tick_bias=12, levels=True)
    assert len(back.frames) == len(rows) and [str(int(o)) for o in back.frames["offset"]] == list(rows)
    at = {int(f["offset"]): (f["bytes"].tobytes(), int(x["kind"]), int(x["signal"])) for f, x in zip(back.frames, back.rx)}
    for o, m in zip((100, 1100, 2100, 3100), msgs):
        assert at[o] == (m.ljust(14, b"\0"), ord("2") if len(m) == 7 else ord("3"), 141), o     # 255 sqrt(10000 / 32768), rounded
    text = A.host_wire_parse(avr.read_bytes(), format="avr", filter=A.WIRE_IN_SHORT, tick_bias=12)
    assert text.frames.tobytes() == back.frames.tobytes() and set(text.rx["kind"].tolist()) == {ord("@")}


def test_replay_beast_alone_keeps_the_records_on_the_device(gpu, tmp_path):
    """tools/replay.py FILE --replies --beast OUT: the list's own lines, and the file's signal bytes from records that
    never came to the host"""
    import os
    import subprocess
    import sys
    from tests.test_replies_tool import capture
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    iq, msgs = capture()
    path, beast = tmp_path / "capture.bin", tmp_path / "out.bin"
    (iq.view(np.uint8) ^ 0x80).tofile(path)
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "replay.py"), str(path), "--replies", "--beast", str(beast)],
                       capture_output=True, text=True, timeout=120, cwd=root)
    assert r.returncode == 0, r.stderr
    rows = r.stdout.splitlines()
    assert f"0.000050 100 replies DF11 {msgs[0].hex().upper()}" in rows and f"0.001050 2100 demod DF17 {msgs[2].hex().upper()}" in rows
    back = A.host_wire_parse(beast.read_bytes(), filter=A.WIRE_IN_SHORT, levels=True)
    assert [str(int(o)) for o in back.frames["offset"]] == [x.split()[1] for x in rows]
    at = {int(f["offset"]): (int(x["kind"]), int(x["signal"])) for f, x in zip(back.frames, back.rx)}
    assert [at[o] for o in (100, 1100, 2100, 3100)] == [(ord("2"), 141), (ord("2"), 141), (ord("3"), 141), (ord("3"), 141)]


# ---- the chain -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("st", ["i8", "i16"])
def test_chain_samples_to_wire_and_back(ctx, st):
    """a buffer with a DF11, a DF4, a DF17 and a DF20, and a DF11 whose 128 samples are the buffer's last: the replies scan,
    the merge with the demodulator's list, the level records where they lie, Beast with the short bit, and wire input
    with its short bit give the merged list back, with the model's signal bytes"""
    d, dtype = ctx[st], DTYPES[st]
    n = 6000
    amp = 100 if st == "i8" else 12000
    iq = RM.noise(n, dtype, 1, RK.LOW)
    msgs = [MM.all_call(0x4B1A2C), MM.reply(4, 0x4B1A2C, field=0x1838), MM.squitter(0xA05629, me=bytes([0x58, 1, 2, 3, 4, 5, 6])),
            MM.reply(20, 0x4B1A2C, field=0x1838, rest=MM.callsign_mb("SWR123__")), MM.all_call(0x4B1A2D)]
    for m, at in zip(msgs, (100, 1100, 2100, 3100, n - 128)):
        RM.render(iq, m, at, pulse=(amp, 0))
    dev = _dev(iq)
    d.demod_device_async(dev.data_ptr(), n)
    found, fcounts, _, flags = d.fetch()
    assert flags == 0 and found["offset"].tolist() == [2100]
    replies, rcounts, _ = d.replies_of(dev.data_ptr(), n_samples=n)
    assert {100, 1100, 3100, n - 128} <= set(replies["offset"].tolist())
    frames, src, counts = d.merge_lists(found, fcounts, replies, rcounts)
    bias = 600
    for levels_from in ("device", "host"):
        if levels_from == "device":
            assert d.levels_modes_of(dev.data_ptr(), n, frames, counts, fetch=False) is None
            lv_arg = d.levels_modes_device()
            records = _records_at(lv_arg, len(frames))
        else:
            records = lv_arg = d.levels_modes_of(dev.data_ptr(), n, frames, counts)
        model = LM.levels(iq, frames)
        assert records.tobytes() == model.tobytes() == A.host_frame_levels_modes(iq, frames).tobytes()
        tail = int(np.nonzero(frames["offset"] == n - 128)[0][0])
        assert int(records[tail]["flags"]) == A.ADSB_LEVEL_VALID | A.ADSB_LEVEL_SHORT and int(records[tail]["signal_sum"]) == 60 * amp * amp
        stream, ends = d.wire_of(frames, lv_arg, tick_bias=bias, short=True)
        _same((stream, ends), LM.encode("beast", frames, model, ST[st], bias), levels_from)
        back = d.wire_in_of(stream, filter=A.WIRE_IN_SHORT, tick_bias=bias, levels=True)
        assert back.frames.tobytes() == frames.tobytes()
        assert back.rx["signal"].tolist() == LM.signal_bytes(model, ST[st]) and min(back.rx["signal"].tolist()) > 0
        assert back.rx["kind"].tolist() == [ord("2") if s else ord("3") for s in K.is_short(frames)]
    del dev
