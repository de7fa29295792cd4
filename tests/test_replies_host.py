"""Mode S replies from samples, CPU tier: the CPU mirror (adsb_host_replies, adsb_host_merge_lists), which compiles the
text the device compiles (air_rs_amd/csrc/adsb_replies.h), byte for byte against the independent NumPy model
(tests/replies_model.py) on every case of tests/replies_cases.py, and the cases' own present / absent lists against
both.  The mutants of profiles/replies_checks.txt are caught here by name."""
import numpy as np
import pytest

import air_rs_amd as A
from tests import replies_cases as K
from tests import replies_model as M

DTYPES = {"i8": np.int8, "i16": np.int16}


def run_host(c):
    return A.host_replies(c["iq"], c["n_channels"], c["n_samples"], c["channel_stride"], **c["kw"])


def same(got, want, what):
    (gf, gc, gh), (wf, wc, wh) = got, want
    assert len(gf) == len(wf) and gf.tobytes() == wf.tobytes(), (what, len(gf), len(wf))
    assert gc.tolist() == wc.tolist(), (what, gc, wc)
    assert gh.tobytes() == wh.tobytes(), (what, gh, wh)


def _cases(st):
    return pytest.mark.parametrize("c", K.all_cases(DTYPES[st]), ids=K.ids(DTYPES[st]))


def _check(c):
    got, want = run_host(c), K.run_model(c)
    same(got, want, c["name"])
    K.check_expectations(c, got[0], got[1])
    if c["kw"].get("max_frames"):                       # the head of the whole list, TRUNCATED, the exact total
        whole = K.run_model(dict(c, kw={k: v for k, v in c["kw"].items() if k != "max_frames"}))
        cut = c["kw"]["max_frames"]
        assert len(whole[0]) > cut and got[0].tobytes() == whole[0][:cut].tobytes()
        assert got[2]["flags"] == A.ADSB_FLAG_TRUNCATED and got[2]["total_found"] == len(whole[0]) and got[2]["n_out"] == cut


@_cases("i8")
def test_mirror_is_the_model_i8(lib, c):
    _check(c)


@_cases("i16")
def test_mirror_is_the_model_i16(lib, c):
    _check(c)


def _named(st, name):
    return next(c for c in K.all_cases(DTYPES[st]) if c["name"] == name)


@pytest.mark.parametrize("st", ["i8", "i16"])
def test_strict_preamble(lib, st):
    """mutant 'strict -> non-strict preamble': a tie between the weakest pulse and the strongest gap is no preamble, one
    unit more is; constant input gives nothing"""
    tie, above = _named(st, "a preamble whose weakest pulse equals its strongest gap"), _named(st, "... and one unit above it")
    f, _, h = run_host(tie)
    assert 40 not in f["offset"].tolist()
    f, _, h = run_host(above)
    assert 40 in f["offset"].tolist() and h["n_preamble"] >= 1
    flat = np.full((5000, 2), 7, dtype=DTYPES[st])
    f, _, h = run_host(K.case("constant", flat))
    assert len(f) == 0 and h.tobytes() == bytes(80)


@pytest.mark.parametrize("st", ["i8", "i16"])
def test_emit_bound(lib, st):
    """mutant 'the emit bound off by one': the last offset a frame fits at is found, the next is not, for both lengths"""
    last, past = _named(st, "edges at last"), _named(st, "edges at last+1")
    f, counts, _ = run_host(last)
    K.check_expectations(last, f, counts)
    f, counts, _ = run_host(past)
    K.check_expectations(past, f, counts)
    for df in (11, 20):                                  # the shortest buffers that hold one frame, and one sample less
        n = K.span(df)
        iq = np.zeros((n, 2), dtype=DTYPES[st])
        M.render(iq, K.message(df), 0)
        assert run_host(K.case("exact", iq))[0]["offset"].tolist() == [0]
        f, _, h = run_host(K.case("short", iq[:n - 1]))
        assert len(f) == 0 and h["n_preamble"] == 1 and h["total_found"] == 0


def test_all_call_syndrome_bound(lib):
    """mutant 'S < 128 -> S <= 128': DF11 with S = 0, 1, 127 is kept, 128 is not and counts as n_parity"""
    c = _named("i8", "DF and syndrome")
    f, counts, h = run_host(c)
    K.check_expectations(c, f, counts)
    assert h["n_all_call"] == 3 and h["n_df18"] == 1 and h["n_parity"] == 2 and h["n_address_parity"] == 0
    assert h["n_preamble"] >= 10 and h["total_found"] == 4


def test_known_lookup_reaches_both_ends(lib):
    """mutant 'the known lookup missing the last entry': addresses at both ends of known[] and address 0, with lists of 0,
    1 and 4096 addresses; n_not_known counts what the filter turned away"""
    want = {"no": (0, 6), "one": (1, 5), "its first": (1, 5), "4096": (4, 2)}
    for name, (kept, turned_away) in want.items():
        c = _named("i8", f"the known filter with {name} addresses")
        f, counts, h = run_host(c)
        K.check_expectations(c, f, counts)
        assert (h["n_address_parity"], h["n_not_known"], len(f)) == (kept, turned_away, kept), name
    f, _, h = run_host(_named("i8", "address/parity frames without the filter"))
    assert (h["n_address_parity"], h["n_not_known"]) == (6, 0)


def test_noise_is_not_empty(lib):
    for st in DTYPES:
        f, _, h = run_host(_named(st, "seeded noise"))
        assert len(f) > 0 and h["n_preamble"] > len(f) and h["n_df18"] == 0


def test_offsets_carry_the_stream_position(lib):
    c = _named("i8", "three channels, a stride above n_samples")
    f, counts, _ = run_host(c)
    assert (counts >= 1).all() and counts.sum() == len(f)
    assert (f["offset"] >= 10**12 + 7).all() and (f["status"] == 0).all() and (f["fixed_bit"] == 0xFF).all()
    short = f[(f["bytes"][:, 0] >> 3) < 16]
    assert len(short) and not short["bytes"][:, 7:].any()           # wire input's short-frame convention


@pytest.mark.parametrize("m", K.merge_cases(), ids=[m[0] for m in K.merge_cases()])
def test_merge_is_the_stable_merge(lib, m):
    """mutant 'the merge tie reversed': on equal offsets list a's frame goes first"""
    _, a, ca, b, cb = m
    gf, gs, gc = A.host_merge_lists(a, ca, b, cb)
    wf, ws, wc = M.merge(a, ca, b, cb)
    assert gf.tobytes() == wf.tobytes() and gs.tolist() == ws.tolist() and gc.tolist() == wc.tolist()


def test_merge_tie_puts_list_a_first(lib):
    _, a, ca, b, cb = K.merge_cases()[0]
    f, src, counts = A.host_merge_lists(a, ca, b, cb)
    assert f["offset"].tolist() == [1, 5, 9, 9, 9, 20, 20, 20, 30] and counts.tolist() == [9]
    B = A.ADSB_MERGE_FROM_B
    assert src.tolist() == [B | 0, 0, 1, 2, B | 1, 3, B | 2, B | 3, B | 4]
    for k, s in enumerate(src.tolist()):                  # src carries a side array along
        assert f[k].tobytes() == (b if s & B else a)[s & ~B].tobytes()
