"""Extended squitter status, CPU tier: the CPU mirror (adsb_host_es) record for record against the independent model
(tests/es_model.py) on the case lists of tests/es_cases.py and on a list of 70 001 frames, the header's totals, the
known answers field by field, adsb_host_es_integrity against the table over every type code, version and supplement
set, and es_physical on the known answers."""
import numpy as np
import pytest

from tests import es_cases as K
from tests import es_model as M
from tests import modes_model as S

CASES = K.all_cases()


@pytest.fixture(scope="module")
def long_list():
    fr = K.random_list(70_001, 99)
    return fr, M.es(fr)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_mirror_is_the_model(lib, case):
    name, fr, _ = case
    M.same(lib.host_es(fr), M.es(fr), name)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_the_cases_show_what_they_claim(case):
    K.claims_hold(case)


def test_known_answers(lib):
    """the frames of the definition: parity 0, and the mirror's own records (not the model's) field by field"""
    fr = M.frame_list(K.KNOWN_FRAMES)
    assert all(S.syndrome(m) == 0 for m in K.KNOWN_FRAMES)
    recs, hdr = lib.host_es(fr)
    for j, (r, want) in enumerate(zip(recs, K.KNOWN_FIELDS)):
        for key, v in want.items():
            if key == "has":
                assert all(int(r["present"]) & M.HAS[k] for k in v), (j, v, r)
            elif key == "lacks":
                assert not any(int(r["present"]) & M.HAS[k] for k in v), (j, v, r)
            elif key == "flags":
                assert int(r["flags"]) == sum(M.FLAG[k] for k in v), (j, v, r)
            elif key in ("half0", "half1"):
                assert int(r["half"][int(key[-1])]) == v, (j, key, r)
            else:
                assert int(r[key]) == v, (j, key, r)
        assert int(r["reserved"]) == 0
    want_states = [0, 0, 1, 2, 1, 1, 0, 1, 1, 0]                     # CATEGORY 1, POSITION 2, ..., OPERATIONAL 1
    assert M.header_dict(hdr) == dict(n=7, n_state=want_states, n_version=[0, 0, 1, 0], reserved=0)


def test_the_long_list(lib, long_list):
    fr, want = long_list
    K.covers_everything(want["recs"])
    got = lib.host_es(fr)
    M.same(got, want, "70 001 frames")
    h = got[1]
    assert int(h["n"]) == 70_001 == int(h["n_state"].sum())
    assert int(h["n_version"].sum()) == int(h["n_state"][M.OPERATIONAL]) and (h["n_version"] > 500).all()
    assert (h["n_state"] > 1000).all() and int(h["n_state"][M.NOT_ES]) > 30_000      # half of it is random bytes
    assert lib.host_es(fr[:0])[1].tobytes() == bytes(128)


def test_a_field_outside_the_mask_is_zero(lib, long_list):
    """on the mirror's records of the long list: every field whose present bit is off is 0, and every byte of a NOT_ES
    or FOREIGN record beside the state"""
    recs = lib.host_es(long_list[0])[0]
    has = lambda name: recs["present"] & M.HAS[name] != 0
    for field, name in (("category", "CATEGORY"), ("nic_b", "NIC_B"), ("nac_v", "NAC_V"), ("emergency", "EMERGENCY"),
                        ("sil_supplement", "SIL_SUPPLEMENT"), ("nac_p", "NAC_P"), ("nic_baro", "NIC_BARO"), ("sil", "SIL"),
                        ("version", "VERSION"), ("nic_a", "NIC_A"), ("length_width", "LENGTH_WIDTH"), ("sda", "SDA"),
                        ("gva", "GVA"), ("nic_c", "NIC_C")):
        assert has(name).any() and (recs[field][~has(name)] == 0).all(), field
    assert (recs["value"][~(has("RC") | has("SELECTED_ALT") | has("RA"))] == 0).all()
    assert (recs["half"][:, 0][~(has("SQUAWK") | has("BARO") | has("RA") | has("CC_OM"))] == 0).all()
    assert (recs["half"][:, 1][~(has("HEADING") | has("CC_OM"))] == 0).all()
    for flag, name in (("INTENT_CHANGE", "VELOCITY_FLAGS"), ("IFR", "VELOCITY_FLAGS"), ("ALT_FMS", "ALT_SOURCE"),
                       ("AUTOPILOT", "MODES"), ("VNAV", "MODES"), ("ALT_HOLD", "MODES"), ("APPROACH", "MODES"), ("LNAV", "MODES"),
                       ("TCAS", "TCAS"), ("HRD", "HRD"), ("TRACK_HEADING", "TRACK_HEADING")):
        assert (recs["flags"][~has(name)] & M.FLAG[flag] == 0).all(), flag
    assert (recs["reserved"] == 0).all() and (recs["flags"] >> len(M.FLAG_NAMES) == 0).all()
    assert (recs["present"] >> len(M.PRESENT_NAMES) == 0).all()
    quiet = recs[recs["state"] <= M.FOREIGN]
    assert (quiet.view(np.uint8).reshape(-1, 32)[:, 1:] == 0).all()


def test_integrity_is_the_table(lib):
    """adsb_host_es_integrity over all TC 0..31 x version 0..7 and unknown x supp 0..7, and the rows of the table spelt
    out here once more in metres"""
    for tc in range(32):
        for version in list(range(8)) + [M.VERSION_UNKNOWN]:
            for supp in range(8):
                assert lib.host_es_integrity(tc, version, supp) == M.integrity(tc, version, supp), (tc, version, supp)
    A, B, Cc = 1, 2, 4
    rows = {(11, 0, A | B): (0, 185.2), (11, 1, A): (9, 75), (11, 1, B): (8, 185.2), (11, 2, A): (8, 185.2), (11, 2, A | B): (9, 75),
            (13, 0, 0): (0, 926), (13, 1, A | B): (6, 1111.2), (13, 1, B): (6, 926), (13, 2, A | B): (6, 1111.2),
            (13, 2, B): (6, 555.6), (13, 2, 0): (6, 926), (13, 2, A): (6, 1111.2),
            (16, 0, 0): (0, 18520), (16, 1, A): (3, 7408), (16, 2, A): (2, 14816), (16, 2, A | B): (3, 7408), (16, 2, 0): (2, 14816),
            (7, 0, A): (0, 185.2), (7, 1, A | Cc): (9, 75), (7, 2, A | Cc): (8, 185.2), (7, 2, A): (9, 75), (7, 2, 0): (8, 185.2),
            (8, 0, A | Cc): (0, 0), (8, 1, A | Cc): (0, 0), (8, 2, A | Cc): (7, 370.4), (8, 2, A): (6, 555.6), (8, 2, Cc): (6, 1111.2),
            (8, 2, 0): (0, 0), (8, 5, A | Cc): (7, 370.4),
            (9, 0, 0): (0, 7.5), (9, 2, 0): (11, 7.5), (20, 1, 7): (11, 7.5), (10, 2, 0): (10, 25), (21, 0, 0): (0, 25),
            (12, 2, 7): (7, 370.4), (14, 1, 0): (5, 1852), (15, 2, 0): (4, 3704), (17, 2, 0): (1, 37040), (17, 0, 0): (0, 37040),
            (5, 2, 0): (11, 7.5), (6, 1, 0): (10, 25), (0, 2, 7): (0, 0), (18, 2, 7): (0, 0), (22, 1, 0): (0, 0), (19, 2, 0): (0, 0),
            (31, 2, 7): (0, 0), (11, 7, A | B): (9, 75), (11, M.VERSION_UNKNOWN, A | B): (0, 185.2)}
    for (tc, version, supp), (nic, metres) in rows.items():
        assert lib.host_es_integrity(tc, version, supp) == (nic, round(10 * metres)), (tc, version, supp)
    # each output is optional
    fn = lib.load().adsb_host_es_integrity
    assert fn(11, 2, 3, None, None) == lib.ADSB_OK


def test_es_physical_on_the_known_answers(lib):
    recs, _ = lib.host_es(M.frame_list(K.KNOWN_FRAMES))
    p = lib.es_physical(recs)
    want = {1: dict(selected_altitude_ft=16992.0, baro_setting_mb=1012.8, selected_heading_deg=95 * 180 / 256),
            4: dict(rc_m=185.2), 5: dict(rc_m=185.2)}
    assert sorted(p) == ["baro_setting_mb", "rc_m", "selected_altitude_ft", "selected_heading_deg"]
    assert all(v.shape == (7,) and v.dtype == np.float64 for v in p.values())
    for j in range(7):
        for key, v in p.items():
            if key in want.get(j, {}):
                assert abs(float(v[j]) - want[j][key]) < 1e-9, (j, key, v[j])
            else:
                assert np.isnan(v[j]), (j, key, v[j])
    assert round(float(p["selected_heading_deg"][1]), 1) == 66.8
    # a value the record does not hold is NaN whatever the field's bytes: altitude none, heading status off
    one = lib.host_es(M.frame_list([M.frame(M.me_target(alt=0, baro=1, heading=None, heading_raw=77)),
                                    M.frame(M.me_tc(18, 0, 0x123456789ABC))]))[0]
    q = lib.es_physical(one)
    assert np.isnan(q["selected_altitude_ft"][0]) and np.isnan(q["selected_heading_deg"][0]) and float(q["baro_setting_mb"][0]) == 800.0
    assert np.isnan(q["rc_m"]).all()                                 # TC 18: unknown
    assert float(lib.es_physical(one[0])["baro_setting_mb"][0]) == 800.0   # one record alone
