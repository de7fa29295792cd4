"""Mode S replies, CPU tier: the CPU mirror (adsb_host_modes) record for record against the independent model
(tests/modes_model.py) on the case lists of tests/modes_cases.py, the cut property at every cut of a 300-frame list, and
the argument checks."""
import ctypes as C

import numpy as np
import pytest

from air_rs_amd import _lib as L
from tests import modes_cases as K
from tests import modes_model as M

CASES = K.all_cases()


def _split(n):
    """three receivers' counts for an n-frame list"""
    return [n // 3, 0, n - n // 3]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_mirror_is_the_model(lib, case):
    name, fr, known = case
    M.same(lib.host_modes(fr, known=known), M.modes(fr, known), name)
    counts = _split(len(fr))
    M.same(lib.host_modes(fr, counts, known), M.modes(fr, known, counts), (name, "with counts"))


def test_the_cases_can_show_a_failure():
    """every kind under every DF that has it, every flag, and the named situations are really in the inputs"""
    seen, flags = set(), 0
    for _, fr, known in CASES:
        recs = M.modes(fr, known)["recs"]
        seen |= set(zip(recs["df"].tolist(), recs["kind"].tolist()))
        flags |= int(np.bitwise_or.reduce(recs["flags"])) if len(recs) else 0
    for df in M.ADDRESS_PARITY:
        assert {(df, M.KNOWN), (df, M.UNKNOWN)} <= seen, df
    assert {(11, k) for k in (M.SELF, M.KNOWN, M.UNKNOWN, M.PARITY)} <= seen
    assert {(df, k) for df in (17, 18) for k in (M.SELF, M.PARITY)} <= seen
    assert {(df, M.UNSUPPORTED) for df in K.UNSUPPORTED_DFS} <= seen
    assert all(flags & f for f in M.ALL_FLAGS), flags
    # the fields case: Gillham and 25 ft altitudes, no altitude from a code without C bits, text and non-text callsigns
    recs = M.modes(*K.fields()[1:])["recs"]
    assert -1200 in recs["altitude_ft"].tolist() and {7700, 7600, 7500, 7777} <= set(recs["squawk"].tolist())
    assert b"KLM1023_" in recs["callsign"].tolist() and b"AB#DEFGH" in recs["callsign"].tolist()
    assert ((recs["callsign"] != b"") & (recs["flags"] & M.CALLSIGN == 0)).any()
    assert ((recs["df"] == 4) & (recs["flags"] & (M.ALT | M.ALT_METRIC) == 0)).any()
    # the bit flips: every one of the 168 is something other than SELF, and both PARITY and other DFs occur
    recs = M.modes(*K.bit_flips()[1:])["recs"]
    assert (recs["kind"] != M.SELF).all() and {M.PARITY, M.UNSUPPORTED} <= set(recs["kind"].tolist())
    # iid: all KNOWN with the address known, all UNKNOWN without, the iid kept either way
    for known, kind in ((True, M.KNOWN), (False, M.UNKNOWN)):
        recs = M.modes(*K.iids(known)[1:])["recs"]
        assert set(recs["kind"].tolist()) == {kind} and recs["iid"].tolist() == list(range(1, 128))
        assert set(recs["address"].tolist()) == {K.A}
    recs = M.modes(*K.self_between()[1:])["recs"]
    assert recs["kind"].tolist() == [M.UNKNOWN, M.SELF, M.KNOWN, M.UNKNOWN, M.SELF, M.KNOWN, M.KNOWN]
    got = M.modes(*K.edge_addresses()[1:])
    assert got["recs"]["kind"].tolist() == [M.UNKNOWN, M.UNKNOWN, M.SELF, M.SELF, M.KNOWN, M.KNOWN, M.KNOWN, M.SELF]
    assert got["known_out"].tolist() == [0, 0xFFFFFF]
    got = M.modes(*K.duplicates()[1:])
    assert got["known_out"].tolist() == sorted([K.A, K.B]) and len(got["squitters"]) == 5


def test_cut_property_at_every_cut(lib):
    """modes(L1, K) then modes(L2, known_out1) == modes(L1 + L2, K): the records and the final known_out"""
    fr, pool = K.random_list(300, 21)
    known = pool[1::3]
    whole = lib.host_modes(fr, known=known)
    M.same(whole, M.modes(fr, known), "whole")
    assert {M.SELF, M.KNOWN, M.UNKNOWN, M.PARITY, M.UNSUPPORTED} == set(whole[0]["kind"].tolist())
    late = [j for j in range(1, 300) if whole[0]["kind"][j] == M.KNOWN and whole[0]["address"][j] not in known.tolist()]
    assert len(late) > 20                                            # addresses learnt inside the list, used after a cut
    for cut in range(301):
        one = lib.host_modes(fr[:cut], known=known)
        two = lib.host_modes(fr[cut:], known=one[1])
        assert np.concatenate([one[0], two[0]]).tobytes() == whole[0].tobytes(), cut
        assert two[1].tolist() == whole[1].tolist(), cut
        assert np.concatenate([one[2], two[2]]).tobytes() == whole[2].tobytes(), cut


def test_bytes_past_the_length_are_ignored(lib):
    fr = M.frame_list([M.reply(4, K.A, field=0x0AB0), M.all_call(K.B), M.reply(5, K.B)])
    dirty = fr.copy()
    dirty["bytes"][:, 7:] = 0xA5
    a, b = lib.host_modes(fr, known=[K.A]), lib.host_modes(dirty, known=[K.A])
    assert a[0].tobytes() == b[0].tobytes() and a[0]["kind"].tolist() == [M.KNOWN, M.SELF, M.KNOWN]
    M.same(b, M.modes(dirty, [K.A]), "dirty tails")


def test_argument_checks(lib):
    fn = L.load().adsb_host_modes
    fr = M.frame_list([K.KNOWN_FRAME] * 3)
    recs = np.zeros(3, dtype=M.REC_DTYPE)

    def call(frames=fr, n=3, counts=None, R=0, known=None, nk=None):
        k = None if known is None else np.array(known, dtype=np.uint32)
        c = None if counts is None else np.array(counts, dtype=np.uint64)
        return fn(None if frames is None else frames.ctypes.data, n, None if c is None else c.ctypes.data, R,
                  None if k is None else k.ctypes.data, (0 if k is None else len(k)) if nk is None else nk,
                  recs.ctypes.data, None, None, None, None)

    assert call() == lib.ADSB_OK and recs["kind"].tolist() == [M.SELF] * 3
    for bad in ([2, 1], [1, 1], [5, 5, 6, 6], [1 << 24], [0, 1 << 24]):                # unsorted, repeated, too large
        assert call(known=bad) == lib.ADSB_E_ARG, bad
    assert call(known=[0, 1, (1 << 24) - 1]) == lib.ADSB_OK
    assert call(frames=None) == lib.ADSB_E_ARG and call(known=None, nk=2) == lib.ADSB_E_ARG
    assert call(frames=None, n=0) == lib.ADSB_OK
    assert call(counts=[1, 1], R=2) == lib.ADSB_E_ARG and call(counts=[4], R=1) == lib.ADSB_E_ARG
    assert call(counts=[3], R=0) == lib.ADSB_E_ARG and call(counts=[0] * 256 + [3], R=257) == lib.ADSB_E_ARG
    assert call(counts=[1, 2], R=2) == lib.ADSB_OK and call(counts=[0] * 255 + [3], R=256) == lib.ADSB_OK
    assert call(n=1 << 32) == lib.ADSB_E_CAPACITY
    assert call(known=[1], nk=(1 << 24) + 1) == lib.ADSB_E_ARG
    assert C.sizeof(L.AdsbModesRec) == 32 and C.sizeof(L.AdsbModesHeader) == 64
