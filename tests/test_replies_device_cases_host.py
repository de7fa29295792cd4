"""The cases for the text only the device compiles (tests/replies_cases.py, device_text_cases and merge_many_channels),
CPU tier: the mirror against the model byte for byte on every one, each case's own present / absent lists, and what the
cases claim to hold, asserted from the model's list: two or three kept frames in one run of offsets, every residue of a
tile, the counted and the unexamined last offsets.  tests/test_gpu_replies_device.py puts the device beside them."""
from collections import Counter

import numpy as np
import pytest

import air_rs_amd as A
from tests import replies_cases as K
from tests import replies_model as M
from tests.test_replies_host import DTYPES, run_host, same


def _cases(st):
    return pytest.mark.parametrize("name", K.device_text_names(DTYPES[st]))


def check_capacity(c, got):
    """the head of the whole list; TRUNCATED iff the list is longer; the exact total; counts clipped to the list"""
    cut = c["kw"]["max_frames"]
    whole = K.run_model(dict(c, kw={k: v for k, v in c["kw"].items() if k != "max_frames"}))
    total = len(whole[0])
    assert got[0].tobytes() == whole[0][:cut].tobytes() and int(got[1].sum()) == min(cut, total)
    assert (int(got[2]["n_out"]), int(got[2]["total_found"])) == (min(cut, total), total)
    assert int(got[2]["flags"]) == (A.ADSB_FLAG_TRUNCATED if total > cut else 0)


def _check(st, name):
    c, want = K.device_text_case(DTYPES[st], name), K.device_text_model(DTYPES[st], name)
    got = run_host(c)
    same(got, want, name)
    K.check_expectations(c, got[0], got[1])
    if "n_preamble" in c:
        assert int(want[2]["n_preamble"]) == c["n_preamble"], name
    if c["kw"].get("max_frames"):
        check_capacity(c, got)


@_cases("i8")
def test_mirror_is_the_model_i8(lib, name):
    _check("i8", name)


@_cases("i16")
def test_mirror_is_the_model_i16(lib, name):
    _check("i16", name)


@pytest.mark.parametrize("st", ["i8", "i16"])
def test_names_are_the_cases_own(lib, st):
    """the tests find a case, and the model's answer to it, by its name"""
    names = [c["name"] for c in K.device_text_cases(DTYPES[st])]
    assert names == K.device_text_names(DTYPES[st]) and len(set(names)) == len(names) and not set(names) & set(K.ids(DTYPES[st]))


def _per_run(st, name):
    """kept frames per run of offsets (one thread's bitmap word) in the model's list of a one-channel case"""
    return Counter((K.device_text_model(DTYPES[st], name)[0]["offset"] // K.run(DTYPES[st])).tolist())


@pytest.mark.parametrize("st", ["i8", "i16"])
def test_crowded_runs_are_crowded(lib, st):
    """every planted group is one run with two or more kept frames; i8 runs hold three; the capacities are where the case
    names say"""
    dt = DTYPES[st]
    c, per_run, R, T = K.device_text_case(dt, "crowded runs"), _per_run(st, "crowded runs"), K.run(dt), K.tile(dt)
    planted = {g[0] // R for g in c["groups"]}
    assert len(planted) == len(c["groups"]) == 11
    assert all(per_run[r] >= 2 for r in planted)
    assert len([r for r in per_run if per_run[r] >= 2]) >= len(planted)
    if st == "i8":
        assert len([r for r in planted if per_run[r] == 3]) >= 4
    threads = {g[0] % T // R for g in c["groups"]}
    assert {63, 127, 191, 255} <= threads and c["groups"][8][-1] % T == T - 1     # a wave's last lane; the tile's last offset
    offsets = K.device_text_model(dt, "crowded runs")[0]["offset"].tolist()
    cuts = K.crowded_cuts(dt)
    word = [offsets.index(o) for o in c["groups"][0]]
    assert word == list(range(word[0], word[0] + len(word)))
    assert (cuts["after a word's first member"], cuts["after a word's second member"]) == (word[0] + 1, word[0] + 2)
    assert offsets[cuts["on a tile's first frame"] - 1] >= T > offsets[cuts["on a tile's first frame"] - 2]
    assert offsets[cuts["inside a tile's last word"] - 1] == c["groups"][8][0] and cuts["the total"] == len(offsets)


@pytest.mark.parametrize("st", ["i8", "i16"])
def test_the_filter_splits_crowded_words(lib, st):
    """with the chosen members' syndromes known, words keep that member alone; with all the others', they lose it alone"""
    dt = DTYPES[st]
    for which in K._which(dt):
        for kept in (True, False):
            c = K.device_text_case(dt, K._known_name(which, kept))
            have = set(K.device_text_model(dt, c["name"])[0]["offset"].tolist())
            alone = 0
            for g in c["groups"]:
                inside = [o in have for o in g]
                pick = K.WHICH[which] % len(g)
                alone += inside == [(k == pick) == kept for k in range(len(g))] and not (which == "middle" and len(g) < 3)
            assert alone >= 4, (which, kept, alone)


@pytest.mark.parametrize("st", ["i8", "i16"])
def test_ragged_lengths_take_every_remainder(lib, st):
    dt = DTYPES[st]
    per = 8 if st == "i8" else 4                             # samples per 16-byte chunk of the device's loads
    assert sorted(n % per for n in K.ragged_lengths(dt)) == list(range(1, per))
    for n in K.ragged_lengths(dt):
        c = K.device_text_case(dt, K._ragged_name(n, 0, dt))
        f, _, h = K.device_text_model(dt, c["name"])
        assert len(f) == 4 and (h["n_all_call"], h["n_df18"], h["n_address_parity"]) == (1, 1, 2)
        last = {bytes(x["bytes"])[:14 if x["bytes"][0] >> 3 >= 16 else 7][-1] & 0xF for x in f}
        assert len(last) > 1                                  # the final bits are not all alike
        f, _, h = K.device_text_model(dt, K._ragged_name(n, 1, dt))
        assert len(f) == 0 and h["n_preamble"] >= 4             # cut by the channel's end: counted, never decided


@pytest.mark.parametrize("st", ["i8", "i16"])
def test_every_tile_keeps_a_frame(lib, st):
    dt = DTYPES[st]
    T = K.tile(dt)
    for n_channels, tiles in K.TILES:
        c = K.device_text_case(dt, K._tiles_name(n_channels, tiles))
        assert {(ch, o // T) for ch, o in c["present"]} == {(ch, i) for ch in range(n_channels) for i in range(tiles)}
        assert len({o % T for _, o in c["present"]}) == len(c["present"])
        assert c["n_samples"] == tiles * T + 25


@pytest.mark.parametrize("st", ["i8", "i16"])
def test_many_channels_counts(lib, st):
    dt = DTYPES[st]
    c = K.device_text_case(dt, "300 channels of 136 samples")
    f, counts, h = K.device_text_model(dt, c["name"])
    fits = [int(k % 17 <= 8 and not (k % 17 == 0 and k > 0)) for k in range(K.MANY)]
    assert counts.tolist() == fits and sum(fits[256:]) > 20 and (h["n_preamble"], h["total_found"]) == (283, sum(fits))
    f, counts, h = K.device_text_model(dt, "300 channels of 26 samples")
    assert not counts.any() and (h["n_preamble"], h["total_found"]) == (200, 0)


@pytest.mark.parametrize("st", ["i8", "i16"])
@pytest.mark.parametrize("kind", list(K.OFFSETS))
def test_every_residue_of_a_tile(lib, st, kind):
    dt = DTYPES[st]
    T = K.tile(dt)
    c = K.device_text_case(dt, K._offsets_name(kind, False))
    f, counts, h = K.device_text_model(dt, c["name"])
    assert len(c["present"]) == T and len({o % T for _, o in c["present"]}) == T
    assert set(f["offset"].tolist()) >= {o for _, o in c["present"]}
    assert c["n_samples"] == K.OFFSETS[kind][0] * T and c["iq"].nbytes <= 4 << 20
    c = K.device_text_case(dt, K._offsets_name(kind, True))
    assert len(c["present"]) + len(c["absent"]) == T and len(c["absent"]) in (T // 4, T // 2)


def test_merge_with_many_channels(lib):
    """the mirror's merge against the model's on 5000 channels, runs of empty ones and one crowded channel"""
    _, a, ca, b, cb = K.merge_many_channels()
    assert len(ca) == 5000 and max(ca) == 600 and not any(ca[:40] + cb[:40] + ca[-55:] + cb[-55:] + ca[2000:2300] + cb[2000:2300])
    assert set(ca) >= {0, 1, 2, 3} and set(cb) >= {0, 1, 2, 3}
    gf, gs, gc = A.host_merge_lists(a, ca, b, cb)
    wf, ws, wc = M.merge(a, ca, b, cb)
    assert gf.tobytes() == wf.tobytes() and gs.tolist() == ws.tolist() and gc.tolist() == wc.tolist()
    at, ties = 0, 0
    for n in wc.tolist():                                     # ascending per channel, ties between the lists, a's first
        o, s = wf["offset"][at:at + n].astype(np.int64), ws[at:at + n]
        assert (np.diff(o) >= 0).all()
        eq = np.diff(o) == 0
        ties += int((eq & ((s[:-1] & M.FROM_B) == 0) & ((s[1:] & M.FROM_B) != 0)).sum())
        assert not (eq & ((s[:-1] & M.FROM_B) != 0) & ((s[1:] & M.FROM_B) == 0)).any()
        at += n
    assert ties > 100
