"""Mode S replies from samples on the device (adsb_replies_of, adsb_fetch_replies, adsb_replies_device,
adsb_merge_lists_of): device == CPU mirror == NumPy model, byte for byte, frames, counts and header alike, on every case
of tests/replies_cases.py (a few tile lengths each, sized from adsb_debug_replies_geometry), then what only the device
has: two runs, lists in device memory, the capacity, the state and argument errors, the chain with the demodulator's
launch and adsb_modes_of, and the tool."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import air_rs_amd as A
from air_rs_amd import _lib as L
from tests import modes_model as MM
from tests import replies_cases as K
from tests import replies_model as M
from tests.test_replies_host import DTYPES, run_host, same
from tests.test_replies_tool import capture

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_CHANNELS = 8
_MODEL = {}


def _dev(arr):
    import torch
    return torch.from_numpy(np.ascontiguousarray(arr)).cuda()


def _st(dtype):
    return A.ADSB_SAMPLE_I8 if np.dtype(dtype) == np.int8 else A.ADSB_SAMPLE_I16


@pytest.fixture(scope="module")
def ctx(gpu):
    made = {}
    for name, dtype in DTYPES.items():
        made[name] = A.AdsbDemod(sample_type=_st(dtype), max_samples=12 * K.tile(dtype), max_out=1 << 15,
                                 max_channels=MAX_CHANNELS, host_staging=False)
    yield made
    for d in made.values():
        d.close()


def model(st, c):
    """the model's answer, computed once per case"""
    key = (st, c["name"])
    if key not in _MODEL:
        _MODEL[key] = K.run_model(c)
    return _MODEL[key]


def run_device(d, c, known_on_device=False):
    kw = dict(c["kw"])
    dev = _dev(c["iq"])
    keep = None
    if known_on_device and kw.get("known") is not None and len(kw["known"]):
        keep = _dev(np.ascontiguousarray(kw["known"], dtype=np.uint32))
        kw["known"] = (keep.data_ptr(), len(c["kw"]["known"]))
    got = d.replies_of(dev.data_ptr(), c["n_channels"], c["n_samples"], c["channel_stride"], **kw)
    del dev, keep
    return got


def _check(ctx, st, c):
    got = run_device(ctx[st], c)
    same(got, run_host(c), c["name"] + ": device against mirror")
    same(got, model(st, c), c["name"] + ": device against model")
    K.check_expectations(c, got[0], got[1])


@pytest.mark.parametrize("c", K.all_cases(np.int8), ids=K.ids(np.int8))
def test_device_is_mirror_is_model_i8(ctx, c):
    _check(ctx, "i8", c)


@pytest.mark.parametrize("c", K.all_cases(np.int16), ids=K.ids(np.int16))
def test_device_is_mirror_is_model_i16(ctx, c):
    _check(ctx, "i16", c)


def _named(st, name):
    return next(c for c in K.all_cases(DTYPES[st]) if c["name"] == name)


@pytest.mark.parametrize("st", ["i8", "i16"])
def test_the_capacity_cuts_inside_a_tile(ctx, st):
    """the first max_frames in order, TRUNCATED, the exact total_found, counts clipped to the list; and a capacity of one"""
    c = _named(st, "dense DF11, the capacity inside a tile")
    whole = model(st, _named(st, "dense DF11"))
    cut = c["kw"]["max_frames"]
    f, counts, h = run_device(ctx[st], c)
    assert f.tobytes() == whole[0][:cut].tobytes() and counts.tolist() == [cut]
    assert (int(h["n_out"]), int(h["total_found"]), int(h["flags"])) == (cut, len(whole[0]), A.ADSB_FLAG_TRUNCATED)
    f, counts, h = run_device(ctx[st], dict(c, kw=dict(max_frames=1)))
    assert f.tobytes() == whole[0][:1].tobytes() and counts.tolist() == [1] and int(h["total_found"]) == len(whole[0])
    three = _named(st, "three channels, a stride above n_samples")
    full = model(st, three)
    f, counts, h = run_device(ctx[st], dict(three, kw=dict(three["kw"], max_frames=int(full[1][0]) + 1)))
    assert f.tobytes() == full[0][:len(f)].tobytes() and counts.tolist() == [int(full[1][0]), 1, 0]
    assert int(h["flags"]) == A.ADSB_FLAG_TRUNCATED and int(h["total_found"]) == len(full[0])


@pytest.mark.parametrize("st", ["i8", "i16"])
def test_noise_twice_and_not_empty(ctx, st):
    c = _named(st, "seeded noise")
    one, two = run_device(ctx[st], c), run_device(ctx[st], c)
    same(one, two, "two runs")
    assert len(one[0]) > 0 and len(one[0]) == len(model(st, c)[0])


def test_more_tiles_than_one_group_of_the_folds(gpu):
    """replies_sums and replies_places take 4096 tiles per workgroup (adsb_kernels.h, kRepliesGroupTiles): 4098 CS16 tiles,
    mostly zeros, with frames in the first tile, in the first group's last tile, across the groups' seam, in the second
    group's first tile and at the very end.  The frames in front of the second group, the header's sums over two groups
    and prefix[n_tiles] show in the list, the counts and the header; the capacity cuts inside the second group."""
    T, group = K.tile(np.int16), 4096
    n = (group + 1) * T + 504
    iq = np.zeros((n, 2), dtype=np.int16)
    at = [5, (group - 1) * T + 7, group * T - 60, group * T + 200, n - K.span(11)]
    for k, (df, o) in enumerate(zip((20, 4, 5, 21, 11), at)):
        M.render(iq, K.message(df, K.AA + k, k), o)
    want = A.host_replies(iq)
    assert set(at) <= set(want[0]["offset"].tolist()) and len(want[0]) < 64
    with A.AdsbDemod(sample_type=A.ADSB_SAMPLE_I16, max_samples=n, max_out=64, host_staging=False) as d:
        dev = _dev(iq)
        same(d.replies_of(dev.data_ptr(), n_samples=n), want, "two groups")
        cut = int(np.searchsorted(want[0]["offset"], group * T + 200)) + 1     # up to and with the second group's first frame
        f, counts, h = d.replies_of(dev.data_ptr(), n_samples=n, max_frames=cut)
        assert f.tobytes() == want[0][:cut].tobytes() and counts.tolist() == [cut]
        assert (int(h["total_found"]), int(h["flags"])) == (len(want[0]), A.ADSB_FLAG_TRUNCATED)
        del dev


def test_known_in_device_memory_and_in_host_memory(ctx):
    for name in ("one", "4096"):
        c = _named("i8", f"the known filter with {name} addresses")
        same(run_device(ctx["i8"], c, known_on_device=True), run_device(ctx["i8"], c), name)
        same(run_device(ctx["i8"], c, known_on_device=True), model("i8", c), name)


def test_results_stay_on_the_device(ctx):
    """adsb_replies_device hands out what adsb_fetch_replies copies, and adsb_modes_of reads the list where it lies"""
    d, c = ctx["i8"], _named("i8", "short frames every 131 samples")
    frames, counts, hdr = run_device(d, c)
    fptr, cptr, hptr = d.replies_device()
    assert fptr and cptr and hptr
    recs = d.modes_of((fptr, len(frames)))[0]
    assert recs.tobytes() == A.host_modes(frames)[0].tobytes()
    merged = d.merge_lists((fptr, len(frames)), counts, np.zeros(0, dtype=A.FRAME_DTYPE), [0])
    assert merged[0].tobytes() == frames.tobytes() and merged[1].tolist() == list(range(len(frames)))


def test_state_and_argument_errors(gpu):
    T = K.tile(np.int8)
    with A.AdsbDemod(max_samples=2 * T, max_out=64, max_channels=2, host_staging=False) as d:
        lib, h = L.load(), d.handle
        hdr, cfg = L.AdsbRepliesHeader(), L.AdsbRepliesCfg()
        assert lib.adsb_fetch_replies(h, None, 0, None, None, C.byref(hdr)) == A.ADSB_E_STATE
        assert lib.adsb_replies_device(h, None, None, None) == A.ADSB_E_STATE
        iq = np.zeros((2 * T + 16, 2), dtype=np.int8)
        M.render(iq, K.message(4), 40)
        dev = _dev(iq)
        p = dev.data_ptr()
        call = lambda cfg=cfg, p=p, nch=1, n=2 * T, stride=2 * T, known=None, nk=0: lib.adsb_replies_of(
            h, C.byref(cfg) if cfg else None, p, nch, n, stride, known, nk)
        assert call(cfg=None) == A.ADSB_E_ARG and call(p=None) == A.ADSB_E_ARG and call(nch=0) == A.ADSB_E_ARG
        assert call(p=p + 2) == A.ADSB_E_ARG                                   # misaligned
        assert call(nch=2, n=T, stride=T + 4) == A.ADSB_E_ARG                  # a stride that is no multiple of 8
        assert call(nch=2, n=T, stride=T - 8) == A.ADSB_E_ARG                  # ... below n_samples
        assert call(cfg=L.AdsbRepliesCfg(4)) == A.ADSB_E_ARG and call(nk=1) == A.ADSB_E_ARG
        two = np.array([7, 7], dtype=np.uint32)
        assert call(known=two.ctypes.data, nk=2) == A.ADSB_E_ARG              # a host list that is not distinct
        assert call(n=25) == A.ADSB_E_SHORT
        assert call(n=2 * T + 8) == A.ADSB_E_CAPACITY
        assert call(nch=3, n=64, stride=64) == A.ADSB_E_CAPACITY and call(cfg=L.AdsbRepliesCfg(0, 0, 1 << 32)) == A.ADSB_E_CAPACITY
        assert lib.adsb_fetch_replies(h, None, 0, None, None, C.byref(hdr)) == A.ADSB_E_STATE    # rejected calls enqueue nothing
        assert call() == A.ADSB_OK
        out = np.zeros(1, dtype=A.FRAME_DTYPE)
        assert lib.adsb_fetch_replies(h, None, 1, None, None, None) == A.ADSB_E_ARG
        n_out = C.c_size_t()
        assert lib.adsb_fetch_replies(h, out.ctypes.data, 1, C.byref(n_out), None, C.byref(hdr)) == A.ADSB_OK
        assert (n_out.value, hdr.n_out, int(out[0]["offset"])) == (1, 1, 40)
        assert call(n=25) == A.ADSB_E_SHORT                                    # ... and leave the earlier result
        assert lib.adsb_fetch_replies(h, None, 0, None, None, C.byref(hdr)) == A.ADSB_OK and hdr.n_out == 1
        f, counts, hd = d.replies_of(p, n_samples=2 * T, first_sample=5, max_frames=0)    # max_frames 0: the ctx's max_out
        assert f["offset"].tolist() == [45] and int(hd["flags"]) == 0
        del dev


@pytest.mark.parametrize("m", K.merge_cases(), ids=[m[0] for m in K.merge_cases()])
def test_merge_on_the_device(ctx, m):
    """host lists and device lists give what the model's stable merge gives: equal offsets (a first), an empty channel,
    either list empty, src[]"""
    _, a, ca, b, cb = m
    d = ctx["i8"]
    want = M.merge(a, ca, b, cb)
    got = d.merge_lists(a, ca, b, cb)
    assert got[0].tobytes() == want[0].tobytes() and got[1].tolist() == want[1].tolist() and got[2].tolist() == want[2].tolist()
    da, db = (_dev(a.view(np.uint8)) if len(a) else None), (_dev(b.view(np.uint8)) if len(b) else None)
    got = d.merge_lists((da.data_ptr() if len(a) else 0, len(a)), ca, (db.data_ptr() if len(b) else 0, len(b)), cb)
    assert got[0].tobytes() == want[0].tobytes() and got[1].tolist() == want[1].tolist() and got[2].tolist() == want[2].tolist()
    del da, db


def test_merge_arguments_on_the_device(ctx):
    lib, h = L.load(), ctx["i8"].handle
    _, a, ca, b, cb = K.merge_cases()[0]
    ca, cb = np.array(ca, dtype=np.uint64), np.array(cb, dtype=np.uint64)
    out = np.full(9, 0xEE, dtype=np.uint8).repeat(24).view(A.FRAME_DTYPE)
    ok = [h, a.ctypes.data, ca.ctypes.data, b.ctypes.data, cb.ctypes.data, 1, out.ctypes.data, None, None]
    for k, v in ((2, None), (4, None), (5, 0), (1, None), (3, None), (6, None)):
        args = list(ok)
        args[k] = v
        assert lib.adsb_merge_lists_of(*args) == A.ADSB_E_ARG, k
    assert out.tobytes() == b"\xee" * 216
    assert lib.adsb_merge_lists_of(*ok) == A.ADSB_OK and out.tobytes() == M.merge(a, ca, b, cb)[0].tobytes()


def test_chain_demod_replies_merge_modes(ctx):
    """the demodulator's launch plus the replies scan on one buffer holding a DF11, then a DF4 and a DF20 of the same
    aircraft, plus a DF17 of another; then merge, then modes_of: the DF11 is SELF, the replies KNOWN, squitters[] holds
    the DF17 only; the demodulator's own list is what it was without the scan"""
    d = ctx["i8"]
    iq, msgs = capture()
    dev = _dev(iq)
    d.demod_device_async(dev.data_ptr(), len(iq))
    found, fcounts, total, flags = d.fetch()
    replies, rcounts, hdr = d.replies_of(dev.data_ptr(), n_samples=len(iq))
    again = d.fetch()[0]
    assert flags == 0 and found.tobytes() == again.tobytes() and found["offset"].tolist() == [2100]
    assert found[0]["bytes"].tobytes() == msgs[2]
    assert not np.isin(2100, replies["offset"]) and {100, 1100, 3100} <= set(replies["offset"].tolist())
    frames, src, counts = d.merge_lists(found, fcounts, replies, rcounts)
    assert counts.tolist() == [len(found) + len(replies)] and (np.diff(frames["offset"].astype(np.int64)) >= 0).all()
    recs, known, squitters, _, mh = d.modes_of(frames)
    by_offset = {int(f["offset"]): r for f, r in zip(frames, recs)}
    assert (int(by_offset[100]["kind"]), int(by_offset[100]["address"])) == (A.ADSB_MODES_SELF, 0x4B1A2C)
    for o in (1100, 3100):
        assert (int(by_offset[o]["kind"]), int(by_offset[o]["address"])) == (A.ADSB_MODES_KNOWN, 0x4B1A2C), o
    assert squitters.tobytes() == found.tobytes() and 0x4B1A2C in known.tolist() and 0xA05629 in known.tolist()
    del dev


def test_replay_prints_the_merged_list(gpu, tmp_path):
    """tools/replay.py FILE --replies --modes on a written capture"""
    iq, msgs = capture()
    path = tmp_path / "capture.bin"
    (iq.view(np.uint8) ^ 0x80).tofile(path)
    run = lambda *more: subprocess.run([sys.executable, os.path.join(ROOT, "tools", "replay.py"), str(path), "--replies", *more],
                                       capture_output=True, text=True, timeout=120, cwd=ROOT)
    r = run("--modes")
    assert r.returncode == 0, r.stderr
    rows = [x for x in r.stdout.splitlines() if x.split()[0] in ("0.000050", "0.000550", "0.001050", "0.001550")]
    assert rows == ["0.000050 DF11 SELF 4B1A2C - - -", "0.000550 DF4 KNOWN 4B1A2C 38000 - -", "0.001050 DF17 SELF A05629 - - -",
                    "0.001550 DF20 KNOWN 4B1A2C 38000 - SWR123"]
    r = run("--modes", "--aircraft")                      # (the plain list's text: tests/test_replies_tool.py)
    assert r.returncode == 0, r.stderr
    table = {row.split("\t")[0]: row.split("\t") for row in r.stdout.splitlines()[1:]}
    assert table["4b1a2c"][7] == "38000" and table["4b1a2c"][-1] == "S" and table["a05629"][-1] == ""
