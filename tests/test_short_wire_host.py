"""Short Mode S frames out, CPU tier: the mirrors adsb_host_frame_levels_modes and adsb_host_wire_encode with
ADSB_WIRE_SHORT against the independent models (tests/levels_modes_model.py; the wire bytes from
tests/wire_in_short_model.py's encoder), byte for byte; the round trip through adsb_host_wire_parse in both directions;
the argument rules; and the tool's new lines."""
import ctypes as C
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import levels_model
from tests import levels_modes_model as LM
from tests import short_wire_cases as K
from tests import wire_in_short_model as WS
from tests import wire_model as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = {"i8": np.int8, "i16": np.int16}
ST = {"i8": W.I8, "i16": W.I16}
FORMATS = ("beast", "avr", "avr_mlat")


def host_levels(lib, c, frames=None):
    return lib.host_frame_levels_modes(c["iq"], c["frames"] if frames is None else frames, c["counts"], c["n_samples"],
                                       c["stride"], c["first"])


# ---- levels ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("st", ["i8", "i16"])
@pytest.mark.parametrize("k", range(len(K.LENGTHS) + 1))
def test_levels_mirror_is_model(lib, st, k):
    c = K.levels_cases(DTYPES[st])[k]
    got = host_levels(lib, c)
    assert got.dtype.itemsize == 32 and got.tobytes() == K.model_levels(c).tobytes(), c["name"]
    K.check_levels_expectations(c, got)
    flags = set(got["flags"].tolist())
    assert flags == ({1, 3} if k == len(K.LENGTHS) else {0, 1, 3} if c["n_samples"] >= 240 else {0, 3}), (c["name"], flags)


@pytest.mark.parametrize("st", ["i8", "i16"])
def test_levels_largest_values(lib, st):
    c = K.levels_cases(DTYPES[st])[-1]
    got = host_levels(lib, c)
    p = 2 * int(np.iinfo(DTYPES[st]).min) ** 2
    assert [int(x) for x in got["signal_sum"]] == [60 * p, 116 * p, 60 * p, 116 * p]
    assert [int(x) for x in got["noise_sum"]] == [68 * p, 124 * p, 68 * p, 124 * p]
    assert set(got["peak"].tolist()) == {p} and got["weak_bits"].tolist() == [56, 112, 56, 112]
    assert got["flags"].tolist() == [3, 1, 3, 1]                       # DF15 at n - 128 and DF16 at n - 240 are inside


@pytest.mark.parametrize("st", ["i8", "i16"])
def test_bytes_behind_a_short_frame_are_never_read(lib, st):
    c = K.levels_case(DTYPES[st], 367)
    garbage = c["frames"].copy()
    short = K.is_short(garbage)
    garbage["bytes"][short, 7:] = 0xFF
    assert short.sum() > 5 and host_levels(lib, c, garbage).tobytes() == host_levels(lib, c).tobytes()
    assert LM.levels(c["iq"], garbage, c["counts"], c["n_samples"], c["stride"], c["first"]).tobytes() == K.model_levels(c).tobytes()


@pytest.mark.parametrize("st", ["i8", "i16"])
def test_a_long_frames_record_is_levels_ofs(lib, st):
    """one channel: the long frames' records are adsb_host_frame_levels' and the 240-sample model's"""
    c = K.levels_case(DTYPES[st], 367)
    n0 = c["counts"][0]
    frames, iq = c["frames"][:n0], c["iq"][:367]
    got = lib.host_frame_levels_modes(iq, frames, first_sample=c["first"])
    old = lib.host_frame_levels(iq, frames, first_sample=c["first"])
    long = ~K.is_short(frames)
    assert long.sum() > 3 and got[long].tobytes() == old[long].tobytes()
    assert got[long].tobytes() == levels_model.levels(iq, frames[long], c["first"]).tobytes()
    assert got.tobytes() == host_levels(lib, c)[:n0].tobytes()


def test_levels_arguments(lib):
    from air_rs_amd import _lib
    L = _lib.load()
    c = K.levels_case(np.int8, 241)
    iq, fr = c["iq"], c["frames"]
    counts = np.array(c["counts"], dtype=np.uint64)
    out = np.full(len(fr) * 32, 0xEE, dtype=np.uint8)
    ok = dict(st=0, iq=iq.ctypes.data, nch=4, n=241, stride=241, first=c["first"], fr=fr.ctypes.data, counts=counts.ctypes.data,
              k=len(fr), out=out.ctypes.data)

    def host(**kw):
        a = dict(ok, **kw)
        return L.adsb_host_frame_levels_modes(a["st"], a["iq"], a["nch"], a["n"], a["stride"], a["first"], a["fr"], a["counts"],
                                              a["k"], a["out"])

    for kw in (dict(st=2), dict(st=-1), dict(iq=None), dict(fr=None), dict(counts=None), dict(out=None), dict(nch=0),
               dict(nch=(1 << 20) + 1), dict(stride=240), dict(k=len(fr) - 1), dict(k=len(fr) + 1)):
        assert host(**kw) == lib.ADSB_E_ARG, kw
    assert (out == 0xEE).all()                                           # untouched by rejected calls
    assert host(k=1 << 32) == lib.ADSB_E_CAPACITY
    zero = np.zeros(4, dtype=np.uint64)
    assert host(fr=None, counts=zero.ctypes.data, k=0, out=None) == lib.ADSB_OK
    assert host() == lib.ADSB_OK and out.tobytes() == K.model_levels(c).tobytes()
    one = np.array([len(fr)], dtype=np.uint64)                           # one channel: the stride is not looked at
    assert host(nch=1, n=4 * 241, stride=5, counts=one.ctypes.data) == lib.ADSB_OK
    # the device entry points without a ctx
    dev = C.c_void_p(77)
    assert L.adsb_levels_modes_of(None, iq.ctypes.data, 4, 241, 241, 0, fr.ctypes.data, counts.ctypes.data, len(fr), None) == lib.ADSB_E_ARG
    assert L.adsb_levels_modes_device(None, C.byref(dev)) == lib.ADSB_E_ARG and dev.value == 77
    assert lib.ADSB_LEVEL_SHORT == _lib.ADSB_LEVEL_SHORT == 2 and lib.ADSB_WIRE_SHORT == _lib.ADSB_WIRE_SHORT == 0x100
    hip = open(os.path.join(ROOT, "include", "adsb_hip.h")).read()
    assert "#define ADSB_LEVEL_SHORT 0x2u" in hip and "#define ADSB_WIRE_SHORT 0x100u" in hip
    for method in ("levels_modes_of", "levels_modes_device"):
        assert callable(getattr(lib.AdsbDemod, method, None)), method


# ---- the signal byte ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("st", ["i8", "i16"])
def test_signal_byte_of_a_short_record_at_every_boundary(lib, st):
    """the smallest sum of every byte s by 60 pulse samples, and one below it; the same sums in a record without SHORT and
    in a SHORT record without the format's bit scale by 116"""
    fs = LM.FULL_SCALE[ST[st]]
    sums = [0, 1, 60 * fs, 60 * fs + 1, 116 * fs, (1 << 64) - 1]
    for s in range(2, 256):
        edge = -(-((2 * s - 1) ** 2 * 60 * fs) // (4 * 255 * 255))
        sums += [edge - 1, edge]
    fr = W.frame_list([0] * len(sums), [bytes([0x20]) + bytes(13)] * len(sums))
    for flags in (3, 1):
        lv = W.level_list(sums, flags)
        want = [LM.signal_byte(x, ST[st]) for x in lv]
        stream = lib.host_wire_encode(fr, lv, sample_type=ST[st], short=True)[0]
        got = [WS.M.read_beast(stream, m)[2][6] for m in WS.M.beast_marks(stream)]
        assert got == want and (flags == 1 or set(got) == set(range(256))), flags
    lv = W.level_list(sums, 3)
    assert lib.host_wire_encode(fr, lv, sample_type=ST[st])[0] == W.encode("beast", fr, lv, ST[st])[0]


# ---- wire --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("mix", ["short", "long", "alternate", "random"])
def test_wire_mirror_is_model(lib, fmt, mix):
    for st in (W.I8, W.I16):
        fr, lv = K.wire_list(700, seed=40 + st, mix=mix, sample_type=st)
        bias = (1 << 48) - 5 if mix == "random" else 77
        want = LM.encode(fmt, fr, lv, st, bias)
        got = lib.host_wire_encode(fr, lv, format=fmt, sample_type=st, tick_bias=bias, short=True)
        assert got[0] == want[0] and got[1].tolist() == want[1].tolist(), (fmt, mix, st)
        assert lib.host_wire_encode(fr, None, format=fmt, tick_bias=bias, short=True)[0] == LM.encode(fmt, fr, None, st, bias)[0]
    sizes = set(np.diff(np.concatenate([[0], want[1]])).tolist())
    if fmt != "beast":
        long_size = 31 if fmt == "avr" else 43
        assert sizes == {"short": {long_size - 14}, "long": {long_size}}.get(mix, {long_size - 14, long_size})
    else:
        assert min(sizes) >= (23 if mix == "long" else 16) and max(sizes) <= (30 if mix == "short" else 44)


def test_without_the_bit_every_byte_is_the_parents(lib):
    """a list with short frames, SHORT records and garbage behind the short frames, encoded without the bit: 14 frame bytes,
    116, exactly tests/wire_model.py's bytes"""
    fr, lv = K.wire_list(500, seed=50)
    fr["bytes"][K.is_short(fr), 7:] = 0x1A
    for fmt in FORMATS:
        got, want = lib.host_wire_encode(fr, lv, format=fmt, tick_bias=9), W.encode(fmt, fr, lv, W.I8, 9)
        assert got[0] == want[0] and got[1].tolist() == want[1].tolist(), fmt
    bits = lv.copy()
    bits["flags"] &= 1
    assert lib.host_wire_encode(fr, bits)[0] == lib.host_wire_encode(fr, lv)[0]


@pytest.mark.parametrize("st", ["i8", "i16"])
def test_the_short_frame_of_nothing_but_1a(lib, st):
    fr, lv, bias = K.hot_short_frame(ST[st])
    stream, ends = lib.host_wire_encode(fr, lv, sample_type=ST[st], tick_bias=bias, short=True)
    assert stream == b"\x1a\x32" + b"\x1a" * 28 == LM.encode("beast", fr, lv, ST[st], bias)[0] and ends.tolist() == [30]
    assert lib.host_wire_encode(fr, None, format="avr", short=True)[0] == b"*" + b"1A" * 7 + b";\n"
    assert lib.host_wire_encode(fr, None, format="avr_mlat", tick_bias=bias, short=True)[0] == b"@" + b"1A" * 13 + b";\n"
    back = lib.host_wire_parse(stream, filter=lib.WIRE_IN_SHORT, tick_bias=bias, sample_type=ST[st], levels=True)
    assert len(back.frames) == 1 and back.frames[0]["bytes"].tobytes() == b"\x1a" * 7 + bytes(7)
    assert (int(back.frames[0]["offset"]), int(back.rx[0]["signal"]), int(back.rx[0]["kind"])) == (1000, 26, ord("2"))


def test_cap_inside_a_short_frame_and_between_frames(lib):
    fr, lv = K.wire_list(40, seed=60, mix="alternate")               # short, long, short, ...
    stream, ends = LM.encode("beast", fr, lv)
    e = [int(x) for x in ends]
    for cap in (0, 15, e[0] - 1, e[0], e[0] + 1, e[1] - 1, e[1], e[2] - 1, e[2], e[19] + 7, len(stream) - 1, len(stream)):
        got, got_ends = lib.host_wire_encode(fr, lv, cap=cap, short=True)
        assert got == stream[:W.whole_frames(ends, cap)] and got_ends.tolist() == e, cap


# ---- the round trip ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
def test_encode_then_parse_gives_the_list_back(lib, fmt):
    for st in (W.I8, W.I16):
        fr, lv = K.wire_list(600, seed=70 + st, sample_type=st)
        bias = 123456789
        stream = lib.host_wire_encode(fr, lv, format=fmt, sample_type=st, tick_bias=bias, short=True)[0]
        back = lib.host_wire_parse(stream, format=fmt, filter=lib.WIRE_IN_SHORT, tick_bias=bias, sample_type=st, levels=True)
        assert int(back.header["n_frames"]) == len(fr) and int(back.header["n_other"]) == 0
        assert back.frames["bytes"].tobytes() == fr["bytes"].tobytes()
        assert (back.frames["status"] == 0).all() and (back.frames["fixed_bit"] == 0xFF).all()
        short = K.is_short(fr)
        if fmt == "avr":
            assert set(back.rx["kind"].tolist()) == {ord("*")}              # (no timestamp: no offsets)
            continue
        assert back.frames["offset"].tolist() == fr["offset"].tolist()
        if fmt == "beast":
            assert back.rx["kind"].tolist() == [ord("2") if s else ord("3") for s in short]
            assert back.rx["signal"].tolist() == LM.signal_bytes(lv, st)
            # wire input's records carry no SHORT flag and encode to the byte they came from
            assert not (back.levels["flags"] & 2).any()
            assert lib.host_wire_encode(back.frames, back.levels, sample_type=st, tick_bias=bias, short=True)[0] == stream


def canonical_beast(rng, n, bias):
    """a stream in the manner of wire_in_short_model.mixed_beast, canonical: types '2' and '3' only, a first message byte
    whose DF has the type's length (else the frame comes back with the other type), timestamps congruent to bias mod 6"""
    parts = []
    for _ in range(n):
        short = bool(rng.integers(0, 2))
        raw = rng.integers(0, 256, size=7 if short else 14)
        raw[rng.integers(0, 6, size=len(raw)) == 0] = 0x1A
        df = int(rng.integers(0, 16)) if short else int(rng.integers(16, 32))
        raw[0] = df << 3 | int(raw[0]) & 7
        t = (6 * int(rng.integers(0, (1 << 48) // 6)) + bias) % (1 << 48)
        if rng.integers(0, 5) == 0:
            t = (0x1A1A1A1A1A1A // 6 * 6 + bias) % (1 << 48)
        s = 0x1A if rng.integers(0, 6) == 0 else int(rng.integers(0, 256))
        parts.append(WS.beast_frame(b"2" if short else b"3", t, s, bytes(raw.astype(np.uint8))))
    return b"".join(parts)


def canonical_avr(rng, n, bias, stamped):
    parts = []
    for _ in range(n):
        short = bool(rng.integers(0, 2))
        raw = rng.integers(0, 256, size=7 if short else 14).astype(np.uint8)
        raw[0] = (int(rng.integers(0, 16)) if short else int(rng.integers(16, 32))) << 3 | int(raw[0]) & 7
        t = (6 * int(rng.integers(0, (1 << 48) // 6)) + bias) % (1 << 48)
        parts.append(WS.avr_line(bytes(raw), t if stamped else None))
    return b"".join(parts)


@pytest.mark.parametrize("fmt", FORMATS)
def test_parse_then_encode_gives_the_stream_back(lib, fmt):
    rng = np.random.default_rng(80)
    bias = 4
    x = canonical_beast(rng, 500, bias) if fmt == "beast" else canonical_avr(rng, 500, bias, fmt == "avr_mlat")
    for st in (W.I8, W.I16):
        back = lib.host_wire_parse(x, format=fmt, filter=lib.WIRE_IN_SHORT, tick_bias=bias, sample_type=st, levels=True)
        assert int(back.header["n_frames"]) == 500 == len(back.frames)
        again = lib.host_wire_encode(back.frames, back.levels, format=fmt, sample_type=st, tick_bias=0 if fmt == "avr" else bias,
                                     short=True)[0]
        assert again == x, (fmt, st)


# ---- arguments -----------------------------------------------------------------------------------------------------------
def test_the_format_rule(lib):
    from air_rs_amd import _lib
    L = _lib.load()
    fr = W.frame_list([0], [bytes([0x20]) + bytes(13)])
    out, n = np.zeros(64, dtype=np.uint8), C.c_size_t()
    sizes = {}
    for fmt in (0, 1, 2, 3, 4, 0xFF, 0x100, 0x101, 0x102, 0x103, 0x1FF, 0x200, 0x300, 0x80000100, 0xFFFFFFFF):
        cfg = _lib.AdsbWireCfg(fmt, 0, 0)
        rc = L.adsb_host_wire_encode(C.byref(cfg), 0, fr.ctypes.data, None, 1, out.ctypes.data, 64, C.byref(n), None)
        assert rc == (lib.ADSB_OK if fmt in (0, 1, 2, 0x100, 0x101, 0x102) else lib.ADSB_E_ARG), hex(fmt)
        if rc == lib.ADSB_OK:
            sizes[fmt] = n.value
        # a NULL ctx is refused before the format is looked at; with a ctx: tests/test_gpu_short_wire.py
        assert L.adsb_wire_of(None, C.byref(cfg), fr.ctypes.data, None, 1, out.ctypes.data, 64, C.byref(n), None) == lib.ADSB_E_ARG
        assert L.adsb_wire_device_async(None, C.byref(cfg)) == lib.ADSB_E_ARG
    assert sizes == {0: 23, 1: 31, 2: 43, 0x100: 16, 0x101: 17, 0x102: 29}
    # wire input's own switch is ADSB_WIRE_IN_SHORT in `filter`: its format does not take the bit
    ends = np.array([16], dtype=np.uint64)
    stream = np.frombuffer(WS.beast_frame(b"2", 0, 0, bytes([0x20]) + bytes(6)), dtype=np.uint8)
    for fmt, want in ((0, lib.ADSB_OK), (0x100, lib.ADSB_E_ARG), (0x101, lib.ADSB_E_ARG), (0x102, lib.ADSB_E_ARG)):
        cfg = _lib.AdsbWireInCfg(fmt, lib.ADSB_WIRE_IN_SHORT, 0, 0, 0, 0)
        assert L.adsb_host_wire_parse(C.byref(cfg), stream.ctypes.data, 16, ends.ctypes.data, 1, None, None, None, 0, None,
                                      None, None, None) == want, hex(fmt)
    for name in ("wire_of", "wire", "wire_async"):
        import inspect
        assert "short" in inspect.signature(getattr(lib.AdsbDemod, name)).parameters, name
    assert "short" in inspect.signature(lib.host_wire_encode).parameters


# ---- the tool ------------------------------------------------------------------------------------------------------------
def _tool():
    spec = importlib.util.spec_from_file_location("replay_tool", os.path.join(ROOT, "tools", "replay.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_replies_level_lines(lib):
    from tests.test_replies_tool import capture
    tool = _tool()
    iq, msgs = capture()
    replies, counts, _ = lib.host_replies(iq)
    keep = np.isin(replies["offset"], [100, 1100, 3100])
    frames = replies[keep]
    tail = frames[:1].copy()
    tail["offset"] = len(iq) - 100                                   # a short frame that does not fit: n/a
    frames = np.concatenate([frames, tail])
    lv = lib.host_frame_levels_modes(iq, frames)
    rows = [r.split("\t") for r in tool.replies_level_lines(lib.ADSB_SAMPLE_I8, frames, lv).splitlines()]
    assert [r[:2] for r in rows] == [["100", "DF11"], ["1100", "DF4"], ["3100", "DF20"], [str(len(iq) - 100), "DF11"]]
    assert rows[3][2:] == ["n/a"] * 4 and all(r[5] == "0" for r in rows[:3])
    model = LM.levels(iq, frames)
    for r, m, pulses, quiet in zip(rows[:3], model, (60, 60, 116), (68, 68, 124)):
        sig = 10 * np.log10(int(m["signal_sum"]) / pulses / 32768)
        noise = 10 * np.log10(int(m["noise_sum"]) / quiet / 32768)
        assert r[2:5] == [f"{sig:.1f}", f"{noise:.1f}", f"{float(f'{sig:.1f}') - float(f'{noise:.1f}'):.1f}"] or \
            r[2:5] == [f"{sig:.1f}", f"{noise:.1f}", f"{sig - noise:.1f}"], r
    assert -8.5 < float(rows[0][2]) < -4.5 and float(rows[0][4]) > 20      # pulses of (100, 0) over noise of +-2
    assert tool.replies_level_lines(lib.ADSB_SAMPLE_I8, frames[:0], lv[:0]) == ""


@pytest.mark.parametrize("args", [("--replies", "--web"), ("--replies", "--es"), ("--replies", "--aircraft"),
                                  ("--replies", "--beast-in"), ("--replies", "--levels", "--aircraft"),
                                  ("--replies", "--levels", "--modes"), ("--replies", "--mlat"),
                                  ("--replies", "--site=1,2"), ("--replies", "--modes", "--commb")])
def test_the_tool_still_refuses(args, tmp_path):
    path = tmp_path / "capture.bin"
    path.write_bytes(bytes(64))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "replay.py"), str(path), *args], capture_output=True,
                       text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 2 and "error:" in r.stderr and r.stdout == "", (args, r.stderr)
