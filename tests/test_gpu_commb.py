"""Comm-B registers on the device (adsb_commb_of, adsb_fetch_commb, adsb_commb_device): every output byte for byte equal
to the CPU mirror's and the independent model's (tests/commb_model.py), on the case lists, at every list size at which
the kernel takes another path -- T frames per workgroup, from adsb_debug_commb_geometry -- with a long list in host and
in device memory, two runs against each other, and in a chain behind wire input and the Mode S stage on one context."""
import ctypes as C

import numpy as np
import pytest

import air_rs_amd as A
from air_rs_amd import _lib
from tests import commb_cases as K
from tests import commb_model as M
from tests import modes_model as S
from tests import wire_in_short_model as W
from tests.test_gpu_correlate import _dev, _read_device

pytestmark = pytest.mark.gpu
CASES = K.all_cases()


def _T():
    t = C.c_uint32()
    assert _lib.load().adsb_debug_commb_geometry(C.byref(t)) == A.ADSB_OK
    return t.value


@pytest.fixture(scope="module")
def ctx(gpu):
    with A.AdsbDemod(max_samples=1 << 16, max_out=1024) as d:
        yield d


@pytest.fixture(scope="module")
def big():
    """one list of 70 001 frames with its model result, shared"""
    fr = K.random_list(70_001, 99)
    return fr, M.commb(fr)


def _device_result(d):
    """the result read where commb_device() says it is, after the stream has drained"""
    got = d.fetch_commb()                                                                      # waits
    recs, hdr = d.commb_device()
    h = _read_device(hdr, M.HEADER_DTYPE, 1)[0]
    assert h.tobytes() == got[1].tobytes()
    return _read_device(recs, M.REC_DTYPE, int(h["n"])), h


def _check(d, fr, want=None, what=""):
    """device == mirror == model; returns the model's result"""
    want = M.commb(fr) if want is None else want
    M.same(d.commb_of(fr), want, (what, "device"))
    M.same(_device_result(d), want, (what, "device arrays"))
    M.same(A.host_commb(fr), want, (what, "mirror"))
    return want


def test_state_before_the_first_call(gpu):
    L = _lib.load()
    with A.AdsbDemod(max_samples=1 << 16, max_out=64) as d:
        assert L.adsb_fetch_commb(d.handle, None, 0, None) == A.ADSB_E_STATE
        assert L.adsb_commb_device(d.handle, None, None) == A.ADSB_E_STATE
        assert L.adsb_commb_of(None, None, 0) == A.ADSB_E_ARG
        assert L.adsb_commb_of(d.handle, None, 1) == A.ADSB_E_ARG
        assert L.adsb_commb_of(d.handle, None, 1 << 32) == A.ADSB_E_ARG
        fr = M.frame_list(K.KNOWN_FRAMES)
        assert L.adsb_commb_of(d.handle, fr.ctypes.data, 1 << 32) == A.ADSB_E_CAPACITY
        assert L.adsb_fetch_commb(d.handle, None, 0, None) == A.ADSB_E_STATE                  # rejected calls are no call
        assert L.adsb_commb_of(d.handle, fr.ctypes.data, len(fr)) == A.ADSB_OK
        assert L.adsb_fetch_commb(d.handle, None, 0, None) == A.ADSB_OK
        assert L.adsb_commb_device(d.handle, None, None) == A.ADSB_OK
        assert L.adsb_fetch_commb(d.handle, None, 2, None) == A.ADSB_E_ARG
        recs, hdr = np.zeros(2, dtype=M.REC_DTYPE), _lib.AdsbCommbHeader()
        assert L.adsb_fetch_commb(d.handle, recs.ctypes.data, 2, C.byref(hdr)) == A.ADSB_OK    # a short fetch
        assert recs.tobytes() == M.commb(fr)["recs"][:2].tobytes() and (hdr.n, hdr.n_one) == (6, 6)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_case_lists(ctx, case):
    name, fr, _ = case
    K.claims_hold(case)
    _check(ctx, fr, what=name)


def test_list_sizes(ctx, big):
    t = _T()
    fr, want = big
    dev_fr = _dev(fr[:2 * t + 4])
    for n in (0, 1, t - 1, t, t + 1, 2 * t + 1):
        _check(ctx, fr[:n], what=n)
        # and where it lies on the device, from the fourth frame on: such a list is 8-byte aligned, not more
        got = ctx.commb_of((dev_fr.data_ptr() + 3 * 24, n))
        M.same(got, dict(recs=want["recs"][3:3 + n], header=M.commb(fr[3:3 + n])["header"]), (n, "device list"))
    K.covers_everything(want["recs"][:2 * t + 4])
    del dev_fr


def test_the_large_list_in_host_and_device_memory_twice(ctx, big):
    fr, want = big
    K.covers_everything(want["recs"])
    assert want["header"]["n_ambiguous"] > 2000 and min(want["header"]["n_bds"]) > 2000 and want["header"]["n_none"] > 5000
    first = ctx.commb_of(fr)
    M.same(first, want, "host list")
    dev_fr = _dev(fr)
    second = ctx.commb_of((dev_fr.data_ptr(), len(fr)))
    M.same(second, want, "device list")
    arrays = _device_result(ctx)
    M.same(arrays, want, "device arrays")
    third = ctx.commb_of((dev_fr.data_ptr() + 24, len(fr) - 1))      # from the second frame on: not 16-byte aligned
    assert third[0].tobytes() == want["recs"][1:].tobytes()
    fourth = ctx.commb_of((dev_fr.data_ptr(), len(fr)))
    again = _device_result(ctx)
    for a, b, c, e in zip(first, second, fourth, again):
        assert a.tobytes() == b.tobytes() == c.tobytes() == e.tobytes()                       # run to run: the same bytes
    del dev_fr


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
    tail = M.commb(frames[(reps - 1) * len(fr):])["header"]
    header = {k: (reps - 1) * want["header"][k] + tail[k] for k in M.HEADER_FIELDS}
    header["n_bds"] = [(reps - 1) * a + b for a, b in zip(want["header"]["n_bds"], tail["n_bds"])]
    header["reserved"] = [0, 0, 0]
    assert header["n"] == n and header["n_one"] > 200_000
    expect = dict(recs=recs, header=header)
    M.same(ctx.commb_of(frames), expect, "host list")
    M.same(_device_result(ctx), expect, "device arrays")
    M.same(A.host_commb(frames), expect, "mirror")


def test_behind_wire_input_and_modes_on_one_context(gpu):
    """Beast bytes with short and long frames -> wire_in_of(short) -> modes_of -> commb_of on wire input's device list:
    records index for index, the known DF20/21 frames with their registers and their addresses"""
    adsb = S.squitter(0x4840D6, me=bytes(range(7)))
    msgs, at = [], {}
    for k, known in enumerate(K.KNOWN_FRAMES):
        address = K.KNOWN[k][1]
        msgs += [S.all_call(address), S.reply(4 + k % 2, address, field=0x0AB0), adsb]
        at[len(msgs)] = k
        msgs.append(known)
    msgs += [M.frame(M.mb_50(gs=250)), M.frame(bytes(7), df=21), S.reply(5, 0x123456, field=0x0AAA)]
    stream = b"".join(W.beast_frame(b"2" if len(m) == 7 else b"3", 6000 * (i + 1), 40 + i, m) for i, m in enumerate(msgs))
    with A.AdsbDemod(max_samples=1 << 16, max_out=1024) as d:
        win = d.wire_in_of(stream, filter="short")
        assert len(win.frames) == len(msgs) and [bytes(f["bytes"].tobytes()[:len(m)]) for f, m in zip(win.frames, msgs)] == msgs
        frames_dev = d.wire_in_device()[0]
        mrec, known_out, squitters, _, mhdr = d.modes_of((frames_dev, len(msgs)))
        crec, chdr = d.commb_of((frames_dev, len(msgs)))
        M.same((crec, chdr), M.commb(win.frames), "the chain")
        assert len(crec) == len(mrec) == len(msgs)
        long_reply = np.isin(mrec["df"], (20, 21))
        assert ((crec["state"] != M.NOT_COMMB) == long_reply).all() and int(chdr["n_commb"]) == long_reply.sum() == 8
        for j, k in at.items():
            _, address, bds, status, value, word = K.KNOWN[k]
            assert (int(mrec["kind"][j]), int(mrec["address"][j])) == (S.KNOWN, address), j   # its all-call came first
            assert (int(crec["state"][j]), int(crec["bds"][j]), int(crec["status"][j])) == (M.ONE, bds, status), j
            assert crec["value"][j].tolist() == value and int(crec["word"][j]) == word, j
        assert crec["state"][-3:].tolist() == [M.AMBIGUOUS, M.EMPTY, M.NOT_COMMB]
        assert bool(mrec["flags"][list(at)[5]] & S.CALLSIGN)                                  # BDS 2,0 both stages see
        # the two stages do not share a result buffer: the modes result fetched after commb_of is what it was
        after = d.fetch_modes()
        assert all(a.tobytes() == b.tobytes() for a, b in zip(after[:3], (mrec, known_out, squitters)))
        assert after[4].tobytes() == mhdr.tobytes()
        assert d.fetch_wire_in().frames.tobytes() == win.frames.tobytes()
        # ... and the other way round, with a list that makes commb_of grow its block
        big = K.random_list(3000, 5)
        d.commb_of(big)
        d.modes_of(big)
        M.same(d.fetch_commb(), M.commb(big), "after modes_of")


def test_replay_prints_the_known_answers(gpu, tmp_path):
    """tools/replay.py FILE --avr-in --modes --commb on an AVR file with the six known answers, each behind its
    aircraft's all-call reply, and a short reply: the tool is what the test is about, so it is started once"""
    import os
    import subprocess
    import sys
    from tests.test_commb_tool import KNOWN_TEXT, ROOT
    lines, t = [], 12_000
    for k, known in enumerate(K.KNOWN_FRAMES):
        for msg in (S.all_call(K.KNOWN[k][1]), known):
            lines.append(W.avr_line(msg, t=t))
            t += 12_000
    lines.append(W.avr_line(S.reply(5, K.KNOWN[0][1], field=0x0AAA), t=t))
    lines.append(W.avr_line(M.frame(M.mb_50(gs=250)), t=t + 12_000))
    path = tmp_path / "known.avr"
    path.write_bytes(b"".join(lines))
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "replay.py"), str(path), "--avr-in", "--modes", "--commb"],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    rows = out.stdout.splitlines()
    assert len(rows) == 14
    for k, text in enumerate(KNOWN_TEXT):
        first, reply = rows[2 * k].split(" "), rows[2 * k + 1].split(" ", 7)
        assert first[1:4] == ["DF11", "SELF", f"{K.KNOWN[k][1]:06X}"] and len(first) == 7           # no Comm-B column
        assert reply[1:4] == [f"DF{K.KNOWN_FRAMES[k][0] >> 3}", "KNOWN", f"{K.KNOWN[k][1]:06X}"] and reply[7] == text, rows[2 * k + 1]
    assert rows[11].split(" ")[6] == "KLM1017"                                                      # BDS 2,0: the Mode S stage's column
    assert rows[12].split(" ")[1:3] == ["DF5", "KNOWN"] and len(rows[12].split(" ")) == 7
    assert rows[13].split(" ", 7)[7] == "?5,0|6,0"
    plain = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "replay.py"), str(path), "--avr-in", "--modes"],
                           capture_output=True, text=True, timeout=120)
    assert plain.returncode == 0 and plain.stdout.splitlines() == [" ".join(r.split(" ")[:7]) for r in rows]
