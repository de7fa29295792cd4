"""CPU tier of the hostile tracker traffic (tests/hostile_traffic.py): the census conditions that keep the GPU tests from
passing without having reached their cases (counted on the oracle alone), the C++ host mirror against the oracle over
that traffic, and the small fixture tests/golden/hostile_traffic.npz.  No GPU needed."""
import math
import os

import numpy as np
import pytest

import air_rs_amd as A
from tests import hostile_traffic as H

SEED = 101                                       # the seed of tests/test_gpu_track_hostile.py


@pytest.mark.parametrize("sps", H.SAMPLE_PERIODS, ids=lambda s: f"{s:.4g}")
def test_census_conditions(oracle, sps):
    """Every named case at least 50 times (the exact latitudes 20), every type code 20 times, at least 50 partners
    exactly at the window of which the oracle accepts 40, per sample period; at most 256 frames of one aircraft in any
    10 s window.  The traffic is deterministic: a second draw is the same bytes."""
    traffic = H.hostile_traffic(oracle, SEED, sps)
    c = H.census(oracle, traffic)
    print(f"census of hostile_traffic(seed={SEED}, sps={sps!r}):\n{H.census_table(c)}")    # shown on failure, or -s
    H.check_census(c)
    again = H.hostile_traffic(oracle, SEED, sps)
    assert again.samples.tobytes() == traffic.samples.tobytes() and again.frames.tobytes() == traffic.frames.tobytes()
    assert (np.diff(traffic.samples.astype(object)) >= 0).all()       # ascending, as the header requires of a list
    assert int(traffic.samples[-1]) > 1 << 53 and int(traffic.samples[0]) == 0


def test_census_counts_what_the_oracle_does(oracle):
    """The census's own restatement of the longitude (for the +-180 count) against the oracle's result, and its
    `refused` against geographic_position, over uniform fields and the generator's chosen pairs."""
    rng = np.random.default_rng(3)
    traffic = H.hostile_traffic(oracle, SEED)
    fields = [tuple(int(x) for x in rng.integers(0, 1 << 17, size=4)) for _ in range(4000)]
    for _, i, j in traffic.cpr_pairs:
        pi, pj = oracle.packet_new(bytes(traffic.frames[i])), oracle.packet_new(bytes(traffic.frames[j]))
        e, o = (pj, pi) if pi.cpr_odd else (pi, pj)
        fields.append((e.cpr_latitude, e.cpr_longitude, o.cpr_latitude, o.cpr_longitude))
    seen = dict.fromkeys(H.CPR_TARGET.values(), 0)
    for f in fields:
        for first_is_odd in (False, True):
            got, want = H.classify(oracle, *f, first_is_odd), oracle.geographic_position(*f, first_is_odd)
            assert got["refused"] == (want is None)
            if want is not None:
                assert got["lon_wrap"] == (not -180.0 <= _raw_longitude(oracle, f, first_is_odd) <= 180.0)
                assert -180.0 <= want[1] <= 180.0
                assert got["lat0"] == (want[0] == 0.0) and got["lat87p"] == (want[0] == 87.0)
                assert got["one_zone"] == (abs(want[0]) > 87.0)
            for k in seen:
                seen[k] += got[k]
    assert min(seen.values()) >= 20, seen


def _raw_longitude(oracle, f, first_is_odd):
    """oracle_calculate_longitude ends with the two +-180 loops; their input is its result plus a multiple of 360,
    recovered here from the zone arithmetic in exact integers."""
    lat = oracle.calculate_latitude(f[0], f[2], first_is_odd)[0]
    nl = oracle.calc_num_zones(lat)
    nz = nl if first_is_odd else max(oracle.calc_num_zones(lat - 1.0), 1)
    m = math.floor((f[1] * (nl - 1) - f[3] * nl) / 131072.0 + 0.5)
    return (360.0 / nz) * (math.fmod(m, nz) + (f[1] if first_is_odd else f[3]) / 131072.0)


def _same_summary(so, sh, where, first_heard=None):
    """The oracle's summary against the mirror's.  An aircraft without a position message yet has no last_contact in
    the oracle (NaN, as the device's records); the mirror keeps the reference's literal value, the time its Aircraft
    was created (aircraft.rs:43), which is the time of its first frame."""
    assert (so.icao, so.callsign, so.altitude, bool(so.has_position)) == \
        (sh.icao, sh.callsign, sh.altitude, bool(sh.has_position)), where
    if so.has_position:
        assert (sh.latitude, sh.longitude) == pytest.approx((so.latitude, so.longitude), abs=1e-12), where
    if math.isnan(so.last_contact):
        assert first_heard is None or sh.last_contact == first_heard, where
    else:
        assert so.last_contact == sh.last_contact, where


@pytest.mark.parametrize("sps", H.SAMPLE_PERIODS, ids=lambda s: f"{s:.4g}")
def test_host_mirror_equals_oracle(oracle, sps):
    """A.Tracker against the oracle's tracker frame by frame: flags and record fields exactly, positions within the
    1e-12 of the other mirror tests; then the whole table."""
    traffic = H.hostile_traffic(oracle, SEED, sps)
    ot, ht = oracle.tracker(), A.Tracker()
    n_new, first_heard = 0, {}
    for k, (fr, t) in enumerate(zip(traffic.frames, traffic.times().tolist())):
        new_o, so = ot.update(bytes(fr), t)
        new_h, sh = ht.update(bytes(fr), t)
        assert new_o == new_h, (k, H.CASES[traffic.case[k]])
        n_new += new_o
        _same_summary(so, sh, (k, H.CASES[traffic.case[k]]), first_heard.setdefault(so.icao, t))
    assert n_new > 2000 and len(ht) == len(ot.aircraft()) == len(np.unique(traffic.icao))
    for so in ot.aircraft():
        _same_summary(so, ht.get(so.icao), hex(so.icao), first_heard[so.icao])


def test_host_cpr_equals_oracle_on_the_chosen_pairs(oracle):
    """A.cpr_position on the field sets the generator chose for a branch, both orders: refusals, the exact
    latitudes, folds, one- and two-zone latitudes, quirk hits and wrapped longitudes."""
    traffic = H.hostile_traffic(oracle, SEED)
    n = {"refused": 0, "decoded": 0}
    for _, i, j in traffic.cpr_pairs:
        pi, pj = oracle.packet_new(bytes(traffic.frames[i])), oracle.packet_new(bytes(traffic.frames[j]))
        e, o = (pj, pi) if pi.cpr_odd else (pi, pj)
        f = (e.cpr_latitude, e.cpr_longitude, o.cpr_latitude, o.cpr_longitude)
        for first_is_odd in (False, True):
            want, got = oracle.geographic_position(*f, first_is_odd), A.cpr_position(*f, first_is_odd)
            assert (want is None) == (got is None), f
            n["refused" if want is None else "decoded"] += 1
            if want is not None:
                assert got == pytest.approx(want, abs=1e-12)
    assert n["refused"] >= 200 and n["decoded"] >= 1500, n


def test_golden_hostile_fixture(oracle):
    """tests/golden/hostile_traffic.npz (written by make_golden.py from the oracle) is what the generator makes from
    H.GOLDEN, and the oracle and the C++ host mirror both reproduce it: per-frame new-position flags, positions, the
    aircraft table.  No larger than tracker_traffic.npz."""
    here = os.path.join(os.path.dirname(__file__), "golden")
    assert os.path.getsize(os.path.join(here, "hostile_traffic.npz")) <= os.path.getsize(
        os.path.join(here, "tracker_traffic.npz"))
    z = np.load(os.path.join(here, "hostile_traffic.npz"))
    made = H.hostile_traffic(oracle, **H.GOLDEN)
    assert float(z["sps"]) == made.sps == H.GOLDEN["sps"]
    assert made.samples.tobytes() == z["samples"].tobytes() and made.frames.tobytes() == z["frames"].tobytes()
    assert set(made.case.tolist()) == set(range(len(H.CASES))) and len({p["region"] for p in made.window_pairs}) == 3
    assert 200 <= len(z["frames"]) <= 600 and 30 <= int(z["new_position"].sum()) < len(z["frames"]) // 2
    ot, ht = oracle.tracker(), A.Tracker()
    times = z["samples"].astype(np.float64) * float(z["sps"])
    for k, (t, fr) in enumerate(zip(times.tolist(), z["frames"])):
        new_o, so = ot.update(bytes(fr), t)
        new_h, sh = ht.update(bytes(fr), t)
        assert new_o == new_h == bool(z["new_position"][k]), k
        if new_o:
            assert (so.latitude, so.longitude) == tuple(z["position"][k])
            assert (sh.latitude, sh.longitude) == pytest.approx(tuple(z["position"][k]), abs=1e-12)
        else:
            assert tuple(z["position"][k]) == (0.0, 0.0)
    table = sorted(ot.aircraft(), key=lambda s: s.icao)
    assert [s.icao for s in table] == list(z["icao"]) and table[0].icao == 0 and table[-1].icao == 0xFFFFFF
    for k, s in enumerate(table):
        sh = ht.get(s.icao)
        assert s.callsign == bytes(z["callsign"][k]) == sh.callsign
        assert s.altitude == z["altitude"][k] == sh.altitude
        assert bool(s.has_position) == bool(z["has_position"][k]) == bool(sh.has_position)
        if s.has_position:
            assert (s.latitude, s.longitude) == (z["latitude"][k], z["longitude"][k])
            assert (sh.latitude, sh.longitude) == pytest.approx((s.latitude, s.longitude), abs=1e-12)
        lc = float(z["last_contact"][k])
        assert (math.isnan(lc) and math.isnan(s.last_contact)) or lc == s.last_contact == sh.last_contact
