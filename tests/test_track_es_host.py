"""The CPU mirror of a table's extended squitter step (adsb_host_es_resolve, adsb_host_track_es_of,
adsb_host_track_es_merge, folded over a list by air_rs_amd.host_track_es) against tests/track_es_model.py, a sequential
model, byte for byte: the per-frame outputs and the 256-byte records.  Every field is an integer or a copied frame time,
so nothing needs a tolerance.  CPU tier."""
import math

import numpy as np
import pytest

from tests import es_model as M
from tests import track_es_cases as K
from tests import track_es_model as T

SPS = K.SPS


def _mirror(lib, case, cuts=(), keyed=False, bases=None, **kw):
    """the case through the mirror, cut at the given list positions -> (frame_es, records)"""
    state, outs, edges = {}, [], [0] + list(cuts) + [len(case["frames"])]
    frames, es, recs = case["frames"].view(lib.FRAME_DTYPE), case["es"].view(lib.ES_DTYPE), case["recs"].view(lib.MODES_DTYPE)
    records = np.zeros(0, dtype=lib.AIRCRAFT_ES_DTYPE)
    for k, (a, b) in enumerate(zip(edges, edges[1:])):
        _, records, out = lib.host_track_es(frames[a:b], es[a:b], recs[a:b] if keyed else None, SPS,
                                            0 if bases is None else bases[k], state=state, **kw)
        outs.append(out)
    return np.concatenate(outs), records


def _both(lib, case, cuts=(), keyed=False, bases=None, **kw):
    want_out, want_recs, table = K.run_model(case, cuts, keyed, bases, **kw)
    out, recs = _mirror(lib, case, cuts, keyed, bases, **kw)
    T.same_frames(out, want_out, (case["name"], cuts))
    T.same_records(recs, want_recs, (case["name"], cuts))
    return out, recs, table


@pytest.fixture(scope="module")
def big():
    case = K.mix(4097)
    out, recs, table = K.run_model(case)
    return case, out, recs, table


@pytest.mark.parametrize("case", K.small_cases(), ids=lambda c: c["name"])
def test_constructed_lists(lib, case):
    K.claims_hold(case)
    # the cases carry the MODEL's adsb_es_rec records; the library's stateless mirror gives the same bytes
    assert lib.host_es(case["frames"].view(lib.FRAME_DTYPE))[0].tobytes() == case["es"].tobytes()
    out, recs, _ = _both(lib, case)
    K.claims_hold(case, out=out)
    _both(lib, case, keyed=True)


def test_known_answers_in_the_record(lib):
    """the record keeps the newest position's resolved values, and every block the aircraft sent"""
    case = K.every_block()
    _, recs, _ = _both(lib, case)
    r = recs[0]
    assert len(recs) == 1 and int(r["n_es"]) == 9 and int(r["n_position"]) == 2
    assert (int(r["nic"]), int(r["rc_dm"]), int(r["position_tc"]), int(r["nic_b"]), int(r["position_supp"])) == (8, 1852, 11, 1, 6 | T.VERSIONED << 1)
    assert (int(r["version"]), int(r["nic_a"]), int(r["nic_c"]), int(r["category"])) == (2, 0, 1, 0xA3)
    assert (int(r["nac_v"]), int(r["velocity_flags"]), int(r["has"])) == (2, 2, 3)       # the velocity's, after the surface status's 5
    assert r["time"].tolist() == [k * K.STEP * SPS for k in (1, 2, 3, 4, 5)]
    assert r["position_time"] == 8 * K.STEP * SPS and r["version_time"] == 3 * K.STEP * SPS and r["nic_a_time"] == r["nic_c_time"] == 2 * K.STEP * SPS
    for k, name in enumerate(T.BLOCKS):
        assert r[name].tobytes() == case["es"][1 + k].tobytes(), name
    phys = lib.aircraft_es_physical(recs)
    assert abs(phys["rc_m"][0] - 185.2) < 1e-9 and phys["selected_altitude_ft"][0] == 32.0 * 531
    assert abs(phys["baro_setting_mb"][0] - 1012.8) < 1e-9 and abs(phys["selected_heading_deg"][0] - 95 * 180 / 256) < 1e-9
    assert lib.aircraft_es_columns(recs)[0] == ["2", "8", "185.2", "10", "2", "1", "7700", "16992"]
    empty = lib.host_track_es_of(np.zeros(1, dtype=lib.ES_DTYPE)[0], np.zeros(1, dtype=lib.FRAME_INTEGRITY_DTYPE)[0])
    assert all(math.isnan(v[0]) for v in lib.aircraft_es_physical(empty).values())
    assert lib.aircraft_es_columns(empty)[0] == ["n/a"] * 8


def test_keyed_path_rejects(lib):
    case = K.keyed_rejects()
    K.claims_hold(case, keyed=True)
    out, recs, table = _both(lib, case, keyed=True)
    assert sorted(table.state) == [K.A] and int(recs["n_es"][0]) == 2 and int(recs["n_position"][0]) == 1


def test_age_edges(lib):
    case = K.age_edges()
    K.claims_hold(case, max_age_s=K.AGE)
    out, _, _ = _both(lib, case, max_age_s=K.AGE)
    assert out["flags"].tolist() == [T.COUNTED, T.COUNTED | T.POSITION | T.VERSIONED, T.COUNTED | T.POSITION | T.VERSIONED | T.STALE_A]
    out, _, _ = _both(lib, case, max_age_s=float(np.nextafter(K.AGE, 0.0)))           # one ulp less: the first is stale too
    assert out["flags"][1] == T.COUNTED | T.POSITION | T.VERSIONED | T.STALE_A and (int(out["nic"][1]), int(out["rc_dm"][1])) == (8, 1852)
    out, _, _ = _both(lib, case, max_age_s=0.0)
    assert out["flags"][1] & T.STALE_A
    far = K.infinite_age()
    K.claims_hold(far, max_age_s=math.inf)
    _both(lib, far, max_age_s=math.inf)
    out, _, _ = _both(lib, far)                                                       # the default: an hour is too old
    assert out["flags"][1] & T.STALE_A and int(out["nic"][1]) == 8


def test_negative_age_is_stale(lib):
    first, base1, second, base2 = K.negative_age()
    both = dict(name="negative age", frames=np.concatenate([first["frames"], second["frames"]]),
                es=np.concatenate([first["es"], second["es"]]), recs=np.concatenate([first["recs"], second["recs"]]), claim=None)
    out, recs, _ = _both(lib, both, cuts=[1], bases=[base1, base2])
    K.claims_hold(second, out=out[1:])
    assert recs["position_time"][0] == 1.0 and recs["nic_a_time"][0] == 10.0 and recs["version_time"][0] == 10.0


def test_a_full_table_counts_nothing_for_the_aircraft_it_turned_away(lib, big):
    case = big[0]
    out, recs, table = _both(lib, case, [1500], max_aircraft=8)          # the mirror's fold with the table's admission
    keys = [int.from_bytes(b[1:4].tobytes(), "big") for b in case["frames"]["bytes"]]
    turned = np.array([k not in table.state for k in keys])
    assert len(recs) == 8 and turned.any() and not out["flags"][turned].any() and not out.view("<u8")[turned].any()
    assert int(recs["n_es"].sum()) == int((out["flags"] & T.COUNTED != 0).sum())


def test_the_mix_reaches_every_row_and_both_stale_flags(lib, big):
    """through the table path, by the model alone; the mirror gives the model's bytes on that list"""
    case, out, recs, table = big
    K.reaches_everything(table)
    assert lib.host_es(case["frames"].view(lib.FRAME_DTYPE))[0].tobytes() == case["es"].tobytes()
    mirror_out, mirror_recs = _mirror(lib, case)
    T.same_frames(mirror_out, out)
    T.same_records(mirror_recs, recs)
    assert {"STALE_A", "STALE_C"} <= table.reached
    assert (out["flags"] == 0).any() and (out["version"] == M.VERSION_UNKNOWN).any()
    for version in (0, 1, 2, 3):
        assert ((out["flags"] & T.POSITION != 0) & (out["version"] == version)).any(), version
    fewer = K.run_model(K.mix(300))[2]                                   # and a list that is too short does not
    with pytest.raises(AssertionError):
        K.reaches_everything(fewer)


def test_every_cut_of_the_twelve_frame_list(lib):
    case = K.twelve()
    n = len(case["frames"])
    assert n == 12
    K.claims_hold(case)
    whole_out, whole_recs, _ = _both(lib, case)
    for a in range(1, n):
        for b in [None] + list(range(a + 1, n)):
            cuts = [a] if b is None else [a, b]
            for keyed in (False, True):
                out, recs = _mirror(lib, case, cuts, keyed)
                T.same_frames(out, whole_out, cuts)
                T.same_records(recs, whole_recs, cuts)
                want_out, want_recs, _ = K.run_model(case, cuts, keyed)
                T.same_frames(want_out, whole_out, cuts)
                T.same_records(want_recs, whole_recs, cuts)


def test_random_cuts_of_4097_frames(lib, big):
    case, whole_out, whole_recs, _ = big
    rng = np.random.default_rng(3)
    out, recs = _mirror(lib, case)
    T.same_frames(out, whole_out)
    T.same_records(recs, whole_recs)
    for size in (2, 40):
        cuts = sorted(set(rng.integers(1, 4097, size=size).tolist()))
        out, recs = _mirror(lib, case, cuts)
        T.same_frames(out, whole_out, cuts)
        T.same_records(recs, whole_recs, cuts)
        want_out, want_recs, _ = K.run_model(case, cuts)
        T.same_frames(want_out, whole_out, cuts)
        T.same_records(want_recs, whole_recs, cuts)


# ---- the combine -------------------------------------------------------------------------------------------------------
def _parts(lib, case):
    """the record of every counted frame of the case alone, from the whole run's per-frame outputs"""
    out = K.run_model(case)[0]
    es = case["es"].view(lib.ES_DTYPE)
    return [lib.host_track_es_of(es[j], out[j].view(lib.FRAME_INTEGRITY_DTYPE), float(int(case["frames"]["offset"][j])) * SPS)
            for j in range(len(out))]


def test_merge_is_associative_with_the_empty_record_as_identity(lib):
    case = K.mix(120, seed=2, n_aircraft=1)
    parts = _parts(lib, case)
    empty = lib.host_track_es_of(np.zeros(1, dtype=lib.ES_DTYPE)[0], np.zeros(1, dtype=lib.FRAME_INTEGRITY_DTYPE)[0])
    assert empty.tobytes() == T.record(T.empty()).tobytes()
    assert all(math.isnan(x) for x in empty["time"]) and math.isnan(empty["position_time"])
    m = lib.host_track_es_merge
    for k in range(0, len(parts) - 2, 3):
        a, b, c = parts[k:k + 3]
        assert m(m(a, b), c).tobytes() == m(a, m(b, c)).tobytes(), k
        assert m(empty, a).tobytes() == a.tobytes() == m(a, empty).tobytes(), k
    folded = empty
    for p in parts:
        folded = m(folded, p)
    _, records, table = K.run_model(case)                 # the mix's short replies have keys of their own and count nothing
    assert folded.tobytes() == records[sorted(table.state).index(0x400000)].tobytes()
    halves = m(empty, empty)
    for lo, hi in ((0, 50), (50, 120)):
        half = empty
        for p in parts[lo:hi]:
            half = m(half, p)
        halves = m(halves, half)
    assert halves.tobytes() == folded.tobytes()


def test_counts_saturate(lib):
    one = _parts(lib, K.build("a position", [K.position(K.A, 11, 1)]))[0]
    assert int(one["n_es"]) == 1 and int(one["n_position"]) == 1
    for start, want in ((T.U32 - 2, T.U32 - 1), (T.U32 - 1, T.U32), (T.U32, T.U32)):
        held = one.copy()
        held["n_es"], held["n_position"] = start, start
        got = lib.host_track_es_merge(held, one)
        assert (int(got["n_es"]), int(got["n_position"])) == (want, want), start
    both = one.copy()
    both["n_es"], both["n_position"] = T.U32 - 2, 5
    other = one.copy()
    other["n_es"], other["n_position"] = 7, T.U32
    got = lib.host_track_es_merge(both, other)
    assert (int(got["n_es"]), int(got["n_position"])) == (T.U32, T.U32)
    model = T.empty()
    model["n_es"] = model["n_position"] = T.U32 - 1
    for _ in range(2):
        T.count(model, K.build("p", [K.position(K.A, 11, 1)])["es"][0], (1852, 0, 255, 2, 3), 0.0)
    assert model["n_es"] == model["n_position"] == T.U32
