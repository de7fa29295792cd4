"""Extended squitter status on the device (adsb_es_of, adsb_fetch_es, adsb_es_device): every output byte for byte equal to
the CPU mirror's and the independent model's (tests/es_model.py), on the case lists, at every list size at which the
kernel takes another path -- T frames per workgroup, from adsb_debug_es_geometry -- with a long list in host and in device
memory, two runs against each other, canaries behind what a call may write, and in a chain behind wire input and the Mode
S stage on one context."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import air_rs_amd as A
from air_rs_amd import _lib
from tests import es_cases as K
from tests import es_model as M
from tests import modes_model as S
from tests import wire_in_short_model as W
from tests.test_gpu_correlate import _hip_runtime, _read_device

pytestmark = pytest.mark.gpu
CASES = K.all_cases()


def _T():
    t = C.c_uint32()
    assert _lib.load().adsb_debug_es_geometry(C.byref(t)) == A.ADSB_OK
    return t.value


@pytest.fixture(scope="module")
def ctx(gpu):
    with A.AdsbDemod(max_samples=1 << 16, max_out=1024) as d:
        yield d


@pytest.fixture(scope="module")
def big():
    """one list of 70 001 frames with its model result, shared"""
    fr = K.random_list(70_001, 99)
    return fr, M.es(fr)


@contextlib.contextmanager
def _on_device(arr):
    """the address of a copy of arr in device memory, from the HIP runtime the library is bound to"""
    hip, ptr, raw = _hip_runtime(), C.c_void_p(), np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
    hip.hipMalloc.argtypes, hip.hipMalloc.restype = [C.POINTER(C.c_void_p), C.c_size_t], C.c_int
    hip.hipFree.argtypes, hip.hipFree.restype = [C.c_void_p], C.c_int
    hip.hipMemcpy.argtypes, hip.hipMemcpy.restype = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int], C.c_int
    assert hip.hipMalloc(C.byref(ptr), len(raw)) == 0
    try:
        assert hip.hipMemcpy(ptr, raw.ctypes.data, len(raw), 1) == 0                          # hipMemcpyHostToDevice
        yield ptr.value
    finally:
        assert hip.hipFree(ptr) == 0


def _device_result(d):
    """the result read where es_device() says it is, after the stream has drained"""
    got = d.fetch_es()                                                                         # waits
    recs, hdr = d.es_device()
    h = _read_device(hdr, M.HEADER_DTYPE, 1)[0]
    assert h.tobytes() == got[1].tobytes()
    return _read_device(recs, M.REC_DTYPE, int(h["n"])), h


def _check(d, fr, want=None, what=""):
    """device == mirror == model; returns the model's result"""
    want = M.es(fr) if want is None else want
    M.same(d.es_of(fr), want, (what, "device"))
    M.same(_device_result(d), want, (what, "device arrays"))
    M.same(A.host_es(fr), want, (what, "mirror"))
    return want


def test_state_and_argument_errors_before_and_after_a_first_call(gpu):
    L = _lib.load()
    with A.AdsbDemod(max_samples=1 << 16, max_out=64) as d:
        assert L.adsb_fetch_es(d.handle, None, 0, None) == A.ADSB_E_STATE
        assert L.adsb_es_device(d.handle, None, None) == A.ADSB_E_STATE
        assert L.adsb_es_of(None, None, 0) == A.ADSB_E_ARG
        assert L.adsb_es_of(d.handle, None, 1) == A.ADSB_E_ARG
        assert L.adsb_es_of(d.handle, None, 1 << 32) == A.ADSB_E_ARG
        fr = M.frame_list(K.KNOWN_FRAMES)
        assert L.adsb_es_of(d.handle, fr.ctypes.data, 1 << 32) == A.ADSB_E_CAPACITY
        assert L.adsb_fetch_es(d.handle, None, 0, None) == A.ADSB_E_STATE                     # rejected calls are no call
        assert L.adsb_es_of(d.handle, fr.ctypes.data, len(fr)) == A.ADSB_OK
        assert L.adsb_fetch_es(d.handle, None, 0, None) == A.ADSB_OK
        assert L.adsb_es_device(d.handle, None, None) == A.ADSB_OK
        assert L.adsb_fetch_es(d.handle, None, 2, None) == A.ADSB_E_ARG
        assert L.adsb_es_of(d.handle, None, 1) == A.ADSB_E_ARG and L.adsb_es_of(d.handle, fr.ctypes.data, 1 << 32) == A.ADSB_E_CAPACITY
        want = M.es(fr)
        M.same(d.fetch_es(), want, "a rejected call leaves the result")
        # a short fetch and a whole one into buffers with canaries on both sides
        for cap in (2, len(fr), len(fr) + 3):
            recs, hdr = np.full((cap + 2) * 32, 0xC5, dtype=np.uint8), np.full(128 + 64, 0xC5, dtype=np.uint8)
            assert L.adsb_fetch_es(d.handle, recs.ctypes.data + 32, cap, C.cast(hdr.ctypes.data + 32, C.POINTER(_lib.AdsbEsHeader))) == A.ADSB_OK
            took = min(cap, len(fr))
            assert recs[32:32 + 32 * took].tobytes() == want["recs"][:took].tobytes()
            assert (recs[:32] == 0xC5).all() and (recs[32 + 32 * took:] == 0xC5).all()
            assert (hdr[:32] == 0xC5).all() and (hdr[160:] == 0xC5).all()
            assert M.header_dict(hdr[32:160].view(M.HEADER_DTYPE)[0]) == want["header"]
        assert L.adsb_es_of(d.handle, None, 0) == A.ADSB_OK                                    # n = 0 needs no list
        M.same(d.fetch_es(), M.es(fr[:0]), "an empty list")


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_case_lists(ctx, case):
    name, fr, _ = case
    K.claims_hold(case)
    _check(ctx, fr, what=name)


def test_list_sizes(ctx, big):
    t = _T()
    fr, want = big
    with _on_device(fr[:2 * t + 4]) as dev_fr:
        for n in (0, 1, t - 1, t, t + 1, 2 * t + 1):
            _check(ctx, fr[:n], what=n)
            # and where it lies on the device, from the fourth frame on: such a list is 8-byte aligned, not more
            got = ctx.es_of((dev_fr + 3 * 24, n))
            M.same(got, dict(recs=want["recs"][3:3 + n], header=M.es(fr[3:3 + n])["header"]), (n, "device list"))
    K.covers_everything(want["recs"][:2 * t + 4])


def test_nothing_is_written_behind_the_list(gpu, big):
    """a context whose block holds 2 T + 1 records is given T + 1 frames: the records behind them and the bytes between
    the record array and the header, filled with a pattern through es_device()'s addresses, are what they were"""
    t = _T()
    fr, want = big
    hip = _hip_runtime()
    hip.hipMemcpy.argtypes, hip.hipMemcpy.restype = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int], C.c_int
    with A.AdsbDemod(max_samples=1 << 16, max_out=64) as d:
        d.es_of(fr[:2 * t + 1])
        recs, hdr = d.es_device()
        first, end = recs + 32 * (t + 1), hdr                        # the header lies behind the records in one block
        assert 32 * t <= end - first <= 32 * t + 256
        pattern = np.full(end - first, 0xC5, dtype=np.uint8)
        assert hip.hipMemcpy(first, pattern.ctypes.data, len(pattern), 1) == 0                 # hipMemcpyHostToDevice
        M.same(d.es_of(fr[:t + 1]), dict(recs=want["recs"][:t + 1], header=M.es(fr[:t + 1])["header"]), "T + 1 frames")
        assert d.es_device() == (recs, hdr)                                                    # the same block
        assert _read_device(first, np.dtype("u1"), len(pattern)).tobytes() == pattern.tobytes()


def test_the_large_list_in_host_and_device_memory_twice(ctx, big):
    fr, want = big
    K.covers_everything(want["recs"])
    assert min(want["header"]["n_state"]) > 1000 and min(want["header"]["n_version"]) > 500
    first = ctx.es_of(fr)
    M.same(first, want, "host list")
    with _on_device(fr) as dev_fr:
        second = ctx.es_of((dev_fr, len(fr)))
        M.same(second, want, "device list")
        arrays = _device_result(ctx)
        M.same(arrays, want, "device arrays")
        third = ctx.es_of((dev_fr + 24, len(fr) - 1))                # from the second frame on: not 16-byte aligned
        assert third[0].tobytes() == want["recs"][1:].tobytes()
        fourth = ctx.es_of((dev_fr, len(fr)))
        again = _device_result(ctx)
    for a, b, c, e in zip(first, second, fourth, again):
        assert a.tobytes() == b.tobytes() == c.tobytes() == e.tobytes()                       # run to run: the same bytes


def test_more_workgroups_than_one_round_of_the_fold(ctx, big):
    """the folding dispatch takes 8 T workgroups' counts per round: 8 T x T + T + 1 frames make it go round twice, with
    a last round that is nearly empty.  The stage is per frame, so the model's result for a list repeated is its
    result repeated, and the long list's is there already"""
    t = _T()
    fr, want = big
    n = 8 * t * t + t + 1
    reps = -(-n // len(fr))
    frames = np.tile(fr, reps)[:n]
    recs = np.tile(want["recs"], reps)[:n]
    tail = M.es(frames[(reps - 1) * len(fr):])["header"]
    header = dict(n=n, reserved=0)
    for key in ("n_state", "n_version"):
        header[key] = [(reps - 1) * a + b for a, b in zip(want["header"][key], tail[key])]
    assert sum(header["n_state"]) == n and header["n_state"][M.TARGET_STATE] > 20_000
    expect = dict(recs=recs, header=header)
    M.same(ctx.es_of(frames), expect, "host list")
    M.same(_device_result(ctx), expect, "device arrays")
    M.same(A.host_es(frames), expect, "mirror")


def test_behind_wire_input_and_modes_on_one_context(gpu):
    """Beast bytes with short and long frames -> wire_in_of(short) -> modes_of -> es_of on the squitter list modes_of
    leaves on the device: records index for index with the squitters, the known answers with their values; and on wire
    input's own list, index for index with the Mode S records"""
    msgs, at = [], {}
    for k, known in enumerate(K.KNOWN_FRAMES):
        msgs += [S.all_call(0x400000 + k), S.reply(4 + k % 2, 0x400000 + k, field=0x0AB0)]
        at[len(msgs)] = k
        msgs.append(known)
    damaged = bytearray(K.KNOWN_FRAMES[1])
    damaged[13] ^= 0x55                                              # a TARGET_STATE frame whose parity fails: no squitter
    msgs += [bytes(damaged), M.frame(K.TARGET_FULL, df=18, low3=2), M.frame(K.TARGET_FULL, df=20), S.reply(5, 0x123456, field=0x0AAA)]
    stream = b"".join(W.beast_frame(b"2" if len(m) == 7 else b"3", 6000 * (i + 1), 40 + i, m) for i, m in enumerate(msgs))
    with A.AdsbDemod(max_samples=1 << 16, max_out=1024) as d:
        win = d.wire_in_of(stream, filter="short")
        assert len(win.frames) == len(msgs) and [bytes(f["bytes"].tobytes()[:len(m)]) for f, m in zip(win.frames, msgs)] == msgs
        frames_dev = d.wire_in_device()[0]
        mrec, known_out, squitters, _, mhdr = d.modes_of((frames_dev, len(msgs)))
        n_sq = int(mhdr["n_squitters"])
        assert n_sq == len(squitters) == len(K.KNOWN_FRAMES) + 1                               # the known answers and the DF18
        erec, ehdr = d.es_of((d.modes_device()[2], n_sq))
        M.same((erec, ehdr), M.es(squitters), "the chain")
        for r, text in zip(erec, K.KNOWN_FIELDS):
            assert int(r["state"]) == text["state"] and int(r["type_code"]) == text["type_code"]
        assert int(erec["value"][1]) == 16992 and erec["half"][1].tolist() == [10128, 95] and int(erec["half"][0][0]) == 6513
        assert int(erec["state"][-1]) == M.FOREIGN and int(ehdr["n_state"][M.NOT_ES]) == 0
        # on wire input's list: index for index with modes_of's records; the stage reads a damaged frame as it stands
        wrec, whdr = d.es_of((frames_dev, len(msgs)))
        M.same((wrec, whdr), M.es(win.frames), "wire input's list")
        assert len(wrec) == len(mrec) == len(msgs)
        assert ((wrec["state"] != M.NOT_ES) == np.isin(mrec["df"], (17, 18))).all()
        for j, k in at.items():
            assert int(mrec["kind"][j]) == S.SELF and wrec[j].tobytes() == erec[k].tobytes(), j
        j = len(msgs) - 4
        assert int(mrec["kind"][j]) == S.PARITY and int(wrec["state"][j]) == M.TARGET_STATE    # the consumer pairs the two
        # the stages do not share a result buffer: the modes result fetched after es_of is what it was
        after = d.fetch_modes()
        assert all(a.tobytes() == b.tobytes() for a, b in zip(after[:3], (mrec, known_out, squitters)))
        assert after[4].tobytes() == mhdr.tobytes()
        assert d.fetch_wire_in().frames.tobytes() == win.frames.tobytes()
        # ... and the other way round, with a list that makes es_of grow its block, beside the Comm-B stage
        more = K.random_list(3000, 5)
        d.es_of(more)
        d.modes_of(more)
        d.commb_of(more)
        M.same(d.fetch_es(), M.es(more), "after modes_of and commb_of")


def test_replay_prints_the_known_answers(gpu, tmp_path):
    """tools/replay.py FILE --avr-in --es on an AVR file with the known answers, a Comm-B reply and a DF18 frame of
    another kind between them: the tool is what the test is about, so it is started once"""
    import os
    import subprocess
    import sys
    from tests.test_es_tool import KNOWN_ADDRESSES, KNOWN_TEXT, ROOT
    msgs = list(K.KNOWN_FRAMES[:3]) + [M.frame(K.TARGET_FULL, df=20)] + list(K.KNOWN_FRAMES[3:]) + [M.frame(K.TARGET_FULL, df=18, low3=6)]
    path = tmp_path / "known.avr"
    path.write_bytes(b"".join(W.avr_line(m, t=12_000 * (i + 1)) for i, m in enumerate(msgs)))
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "replay.py"), str(path), "--avr-in", "--es"],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    rows = out.stdout.splitlines()
    assert [r.split(" ", 3)[1:] for r in rows[:7]] == [["DF17", a, t] for a, t in zip(KNOWN_ADDRESSES, KNOWN_TEXT)], rows
    assert len(rows) == 8 and rows[7].split(" ", 3)[1:] == ["DF18", "4840D6", "FOREIGN"]      # no line for the Comm-B reply
    assert [float(r.split(" ")[0]) for r in rows[:3]] == [0.001, 0.002, 0.003]
