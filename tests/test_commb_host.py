"""Comm-B registers, CPU tier: the CPU mirror (adsb_host_commb) record for record against the independent model
(tests/commb_model.py) on the case lists of tests/commb_cases.py and on a list of 20 000 frames, the header's totals,
adsb_host_commb_as for every candidate of every ambiguous frame, and commb_physical on the known answers."""
import numpy as np
import pytest

from tests import commb_cases as K
from tests import commb_model as M
from tests import modes_model as S

CASES = K.all_cases()


@pytest.fixture(scope="module")
def long_list():
    fr = K.random_list(20_000, 11)
    return fr, M.commb(fr)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_mirror_is_the_model(lib, case):
    name, fr, _ = case
    M.same(lib.host_commb(fr), M.commb(fr), name)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_the_cases_show_what_they_claim(case):
    K.claims_hold(case)


def test_known_answers(lib):
    """the six frames of the definition: address from the parity, one candidate each, the values"""
    recs, hdr = lib.host_commb(M.frame_list(K.KNOWN_FRAMES))
    for r, (text, address, bds, status, value, word) in zip(recs, K.KNOWN):
        assert S.syndrome(bytes.fromhex(text)) == address
        assert (int(r["state"]), int(r["bds"]), int(r["n_candidates"]), int(r["candidates"])) == (M.ONE, bds, 1, M.BIT[bds]), text
        assert (int(r["status"]), r["value"].tolist(), int(r["word"]), int(r["reserved"])) == (status, value, word, 0), text
    assert M.header_dict(hdr) == dict(n=6, n_commb=6, n_empty=0, n_none=0, n_one=6, n_ambiguous=0,
                                      n_bds=[1, 1, 1, 0, 1, 1, 1], reserved=[0, 0, 0])


def test_the_long_list(lib, long_list):
    fr, want = long_list
    K.covers_everything(want["recs"])
    got = lib.host_commb(fr)
    M.same(got, want, "20 000 frames")
    h = got[1]
    assert int(h["n"]) == 20_000 == int(h["n_commb"]) + int((want["recs"]["state"] == M.NOT_COMMB).sum())
    assert int(h["n_commb"]) == int(h["n_empty"]) + int(h["n_none"]) + int(h["n_one"]) + int(h["n_ambiguous"])
    assert int(h["n_bds"].sum()) == int(h["n_one"]) and (h["n_bds"] > 100).all() and int(h["n_ambiguous"]) > 500
    assert lib.host_commb(fr[:0])[1].tobytes() == bytes(128)


def test_random_payloads_pass_rarely(lib):
    """uniformly random MB: the mirror and the model agree on which of 100 000 draws pass something"""
    rng = np.random.default_rng(3)
    fr = np.zeros(100_000, dtype=M.FRAME_DTYPE)
    fr["bytes"] = rng.integers(0, 256, size=(len(fr), 14)).astype(np.uint8)
    fr["bytes"][:, 0] = 20 << 3
    recs, hdr = lib.host_commb(fr)
    hit = np.flatnonzero(recs["state"] != M.NONE)
    assert 100 < len(hit) < 500 and int(hdr["n_none"]) == len(fr) - len(hit)
    pick = np.concatenate([hit, np.arange(0, len(fr), 50)])
    assert recs[pick].tobytes() == M.commb(fr[pick])["recs"].tobytes()


def test_commb_as_settles_every_ambiguous_frame(lib, long_list):
    fr, want = long_list
    amb = np.flatnonzero(want["recs"]["state"] == M.AMBIGUOUS)[:150]
    rows = [f["bytes"].tobytes() for f in K.ambiguous()[1]] + [fr["bytes"][j].tobytes() for j in amb]
    seen = set()
    for b in rows:
        cand = M.candidates(M.MB(b[4:11]))
        assert len(cand) >= 2
        seen.add(tuple(cand))
        for bds in M.REGISTERS:
            if bds in cand:
                got = lib.host_commb_as(b, bds)
                assert got.tobytes() == np.array([M.record(b, as_bds=bds)], dtype=M.REC_DTYPE).tobytes(), (b.hex(), hex(bds))
                assert int(got["state"]) == M.ONE and int(got["bds"]) == bds and int(got["n_candidates"]) == len(cand)
            else:
                with pytest.raises(lib.AdsbError) as e:
                    lib.host_commb_as(b, bds)
                assert e.value.code == lib.ADSB_E_ARG
    assert {(0x50, 0x60), (0x17, 0x40), (0x40, 0x50, 0x60)} <= seen
    # a frame with one candidate reads as that one only; the inference's own record comes back
    for text, _, bds, *_ in K.KNOWN:
        b = bytes.fromhex(text)
        assert lib.host_commb_as(b, bds).tobytes() == lib.host_commb(M.frame_list([b]))[0][0].tobytes()


def test_commb_physical_on_the_known_answers(lib):
    recs, _ = lib.host_commb(M.frame_list(K.KNOWN_FRAMES + [M.frame(M.mb_50(gs=250))]))
    p = lib.commb_physical(recs)
    want = {0: dict(mcp_altitude_ft=3008.0, fms_altitude_ft=3008.0, baro_setting_mb=1020.0),
            1: dict(roll_deg=12 * 45 / 256, true_track_deg=650 * 90 / 512, ground_speed_kt=438.0, track_rate_deg_s=0.125,
                    true_airspeed_kt=424.0),
            2: dict(magnetic_heading_deg=243 * 90 / 512, ias_kt=252.0, mach=0.42, baro_rate_ft_min=-1920.0,
                    inertial_rate_ft_min=-1920.0)}
    assert len(p) == 13 and all(v.shape == (7,) and v.dtype == np.float64 for v in p.values())
    for j in range(7):
        for key, v in p.items():
            if key in want.get(j, {}):
                assert abs(float(v[j]) - want[j][key]) < 1e-9, (j, key, v[j])
            else:
                assert np.isnan(v[j]), (j, key, v[j])                # another register, 1,7 / 1,0 / 2,0, or AMBIGUOUS
    assert round(float(p["roll_deg"][1]), 2) == 2.11 and round(float(p["true_track_deg"][1]), 2) == 114.26
    assert round(float(p["magnetic_heading_deg"][2]), 2) == 42.71
    # and back: the raw values from the physical ones
    assert round(float(p["baro_setting_mb"][0]) * 10) == int(recs["value"][0][2]) == 10200
    assert round(float(p["mach"][2]) / 0.004) == int(recs["value"][2][2]) == 105
    # a status bit that is off: NaN, whatever the value
    one = lib.host_commb(M.frame_list([M.frame(M.mb_60(ias=300, inertial=-100))]))[0]
    q = lib.commb_physical(one)
    assert float(q["ias_kt"][0]) == 300.0 and float(q["inertial_rate_ft_min"][0]) == -3200.0
    assert np.isnan(q["mach"][0]) and np.isnan(q["magnetic_heading_deg"][0]) and np.isnan(q["baro_rate_ft_min"][0])
