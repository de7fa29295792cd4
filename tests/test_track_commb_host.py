"""The CPU mirror of a track table's Comm-B side (adsb_host_commb_settle, adsb_host_commb_reference,
adsb_host_track_commb_of, adsb_host_track_commb_merge) against tests/track_commb_model.py: on every case list, and with
every check of the rule at its last passing and first failing value.  No device."""
import itertools
import math

import numpy as np
import pytest

import air_rs_amd as A
from tests import commb_cases as CK
from tests import commb_model as CM
from tests import track_commb_cases as K
from tests import track_commb_mirror as MI
from tests import track_commb_model as T

U32 = 2 ** 32 - 1


def stateless(mb):
    """(14 bytes, the model's stateless record) of a DF20 reply with this MB"""
    msg = K.reply(mb)
    return msg, CM.commb([msg])["recs"][0]


def ref_of(msg, time=0.0):
    """(the mirror's reference record, the model's reference dict) of a velocity frame"""
    return A.host_commb_reference(msg, time), T.velocity_of(msg, time)


def both_ways(mb, ref_msg, t=1.0, ref_time=0.0, **cfg):
    """mirror and model on one payload against one reference (None: none); asserts they agree -> (state, bds)"""
    msg, rec = stateless(mb)
    full = dict(T.DEFAULT_CFG, **cfg)
    if ref_msg is None:
        r_lib, r_model = None, None
    else:
        r_lib, r_model = ref_of(ref_msg, ref_time)
        assert (r_model is None) == (int(r_lib["subtype"]) == 0)
        if r_model is not None:                           # the held form of the same reference reads the same
            held = T.velocity_of_record(r_lib)
            assert {k: v for k, v in held.items() if k != "time"} == {k: v for k, v in r_model.items() if k != "time"}
            assert held["time"] == r_model["time"] or math.isnan(ref_time)
    got = A.host_commb_settle(msg, rec, r_lib, t, **full)
    want = T.settle(msg, rec, r_model, t, full)
    assert got.tobytes() == want.tobytes(), (got, want)
    if int(got["state"]) != T.SETTLED:
        assert got.tobytes() == rec.tobytes()
    else:
        assert got["candidates"] == rec["candidates"] and got["n_candidates"] == rec["n_candidates"]
        assert got.tobytes() == np.array(A.host_commb_as(msg, int(got["bds"])), dtype=A.COMMB_DTYPE).tobytes()[:1].replace(
            bytes([T.ONE]), bytes([T.SETTLED])) + got.tobytes()[1:]
    return int(got["state"]), int(got["bds"])


SETTLED_50, SETTLED_60, STAYS = (T.SETTLED, 0x50), (T.SETTLED, 0x60), (T.AMBIGUOUS, 0)
V5 = CM.values(CM.MB(K.BOTH), 0x50)[1]        # roll, track, ground speed, rate, true airspeed of BOTH read as 5,0
V6 = CM.values(CM.MB(K.BOTH), 0x60)[1]
# a 6,0 payload that also reads as 5,0: heading 2040 or 2041 (across the 2047 / 0 wrap), both vertical rates 320 ft/min
HEAD_EVEN, HEAD_ODD = CM.mb_60(heading=-8, baro=10, inertial=10), CM.mb_60(heading=-7, baro=10, inertial=10)


@pytest.fixture(scope="module")
def the_mix():
    case = K.mix()
    return case, K.run_model(case)


def test_constructed_payloads_are_what_they_claim():
    for mb in (K.BOTH, HEAD_EVEN, HEAD_ODD):
        rec = stateless(mb)[1]
        assert int(rec["state"]) == T.AMBIGUOUS and int(rec["candidates"]) == T.C50 | T.C60
    assert V5[1] >> 7 == 11 and V5[2] == 430 and V5[4] == 360 and V6[4] == 5760
    assert CM.values(CM.MB(HEAD_EVEN), 0x60)[1][0] == 2040 and CM.values(CM.MB(HEAD_ODD), 0x60)[1][0] == 2041


@pytest.mark.parametrize("case", K.small_cases(), ids=lambda c: c["name"])
def test_mirror_equals_model_on_the_lists(case):
    K.claims_hold(case)
    out, records, _ = K.run_model(case)
    got_out, got_records = MI.run(case)
    T.same_frames(got_out, out, case["name"])
    T.same_records(got_records, records, case["name"])
    n = len(case["frames"])
    for cuts in ([n // 2], [1, n - 1], list(range(1, n, max(1, n // 7)))):
        cuts = sorted(set(c for c in cuts if 0 < c < n))
        o2, r2 = MI.run(case, cuts=cuts)
        T.same_frames(o2, out, (case["name"], cuts))
        T.same_records(r2, records, (case["name"], cuts))


def test_the_realistic_mix(the_mix):
    case, (out, records, _) = the_mix
    K.claims_hold(case)
    tally = K.mix_tally(case, out)
    print(tally)
    assert tally[0x50]["right"] >= 200 and tally[0x60]["right"] >= 20
    assert tally[0x50]["wrong"] == 0 and tally[0x60]["wrong"] == 0
    got_out, got_records = MI.run(case)
    T.same_frames(got_out, out)
    T.same_records(got_records, records)


def test_held_reference_and_the_lists_own():
    first, second = K.held()
    for cases, want in (((first, second), SETTLED_50), ((first, K.list_wins()), STAYS)):
        model, mirror = T.Table(), MI.Table()
        for c in cases:
            out = model.update(c["frames"], c["recs"], c["commb"])
            T.same_frames(mirror.update(c["frames"], c["recs"], c["commb"]), out)
        assert (int(out["state"][-1]), int(out["bds"][-1])) == want
        T.same_records(mirror.records(), model.records())


# ---- every check at its boundary -----------------------------------------------------------------------------------------
def test_ground_speed_at_s():
    g, S = V5[2], 40
    level = dict(vr=0)
    for ew, want in ((-(g + S), SETTLED_50), (-(g + S + 1), STAYS), (-(g - S), SETTLED_50), (-(g - S - 1), STAYS)):
        assert both_ways(K.BOTH, K.ground_frame(K.A, ew, 0, **level)) == want, ew
    # ground speed below S: the lower bound is 0, and a reference that stands still passes it (its track is not checked)
    for ew, ns in ((-1, 0), (0, 0), (-1, -1)):
        assert both_ways(K.BOTH, K.ground_frame(K.A, ew, ns, **level), max_speed_diff_kt=g + 1) == SETTLED_50
    assert both_ways(K.BOTH, K.ground_frame(K.A, -413, -120, **level), max_speed_diff_kt=U32) == SETTLED_50
    assert both_ways(K.BOTH, K.ground_frame(K.A, -413, -120, **level), max_speed_diff_kt=0) == STAYS   # 430.08 kt
    assert both_ways(K.BOTH, K.ground_frame(K.A, -430, 0, **level), max_speed_diff_kt=0) == SETTLED_50


def test_vertical_rates_at_v():
    # a payload whose 6,0 reading has nothing but the heading and the two rates, 320 and 320 ft/min
    for vr, V, want in ((1344, 1024, SETTLED_60), (1344, 1023, STAYS), (-704, 1024, SETTLED_60), (-704, 1023, STAYS)):
        ref = K.air_frame(K.A, heading=0, airspeed=300, tas=1, vr=vr)       # 5,0's true airspeed of 20 kt fails
        assert both_ways(HEAD_EVEN, ref, max_vrate_diff_fpm=V) == want, (vr, V)


def test_heading_distance_across_the_wrap():
    far = dict(airspeed=300, tas=1)                       # contradicts the 5,0 reading (true airspeed 20 kt)
    assert both_ways(HEAD_EVEN, K.air_frame(K.A, heading=60, **far)) == SETTLED_60        # |2040 - 120| = 128
    assert both_ways(HEAD_ODD, K.air_frame(K.A, heading=61, **far)) == STAYS              # |2041 - 122| = 129
    assert both_ways(HEAD_ODD, K.air_frame(K.A, heading=60, **far)) == SETTLED_60         # 127
    assert both_ways(HEAD_EVEN, K.air_frame(K.A, heading=61, **far)) == STAYS             # 130
    assert both_ways(HEAD_EVEN, K.air_frame(K.A, heading=956, **far)) == SETTLED_60       # 2040 - 1912 = 128
    assert both_ways(HEAD_ODD, K.air_frame(K.A, heading=956, **far)) == STAYS             # 129
    assert both_ways(HEAD_EVEN, K.air_frame(K.A, heading=1020, st=4, airspeed=300, tas=1)) == SETTLED_60


def test_airspeeds_at_s():
    # 5,0's true airspeed against ST 3 with TAS: BOTH says 360 kt; its 6,0 reading fails on the climb of 5760 ft/min
    for airspeed, S, want in ((400, 40, SETTLED_50), (401, 40, STAYS), (320, 40, SETTLED_50), (319, 40, STAYS),
                              (360, 0, SETTLED_50)):
        assert both_ways(K.BOTH, K.air_frame(K.A, airspeed=airspeed, tas=1, vr=0), max_speed_diff_kt=S) == want
    # 6,0's indicated airspeed against ST 3 with IAS.  Such a reference applies no check to the 5,0 reading (its airspeed
    # check needs a true airspeed), so 5,0 is neither supported nor contradicted and the frame stays ambiguous whatever
    # the IAS check says: the check can only be seen to agree between mirror and model
    mb = CM.mb_60(heading=-7, ias=250, baro=10, inertial=10)
    rec = stateless(mb)[1]
    assert int(rec["state"]) == T.AMBIGUOUS and int(rec["candidates"]) == T.C50 | T.C60
    for airspeed, S in ((290, 40), (291, 40), (210, 40), (209, 40), (250, 0), (251, 0)):
        assert both_ways(mb, K.air_frame(K.A, heading=1020, airspeed=airspeed, tas=0), max_speed_diff_kt=S) == STAYS


REF_VECTORS = sorted({(sa * a, sb * b) for a, b in ((407, 985), (408, 985), (409, 985), (984, 985), (985, 985), (985, 984),
                                                     (985, 407), (985, 408), (985, 409), (0, 500), (500, 0), (1, 1), (0, 1),
                                                     (1, 0), (300, 301), (301, 300))
                      for sa in (1, -1) for sb in (1, -1)})


def test_sector16_at_both_comparisons_in_every_sector():
    seen = set()
    for ew, ns in REF_VECTORS:
        k = T.sector16(ew, ns)
        seen.add(k)
        if 985 * abs(ew) != 408 * abs(ns) and abs(ew) != abs(ns) and 408 * abs(ew) != 985 * abs(ns):
            assert k == int((math.degrees(math.atan2(ew, ns)) % 360) // 22.5), (ew, ns)   # tan 22.5 = 0.41421 ~ 408/985
    assert seen == set(range(16))
    # payloads whose 5,0 track lies in the middle of a sector and which still read as 6,0 too: sectors 8 to 11
    tracks = [s * 128 + 64 for s in range(16)]
    payloads = [CM.mb_50(roll=-33, track=t - 2048 if t >= 1024 else t, gs=215, rate=-20, tas=180) for t in tracks]
    payloads = [mb for mb in payloads if int(stateless(mb)[1]["candidates"]) == T.C50 | T.C60
                and int(stateless(mb)[1]["state"]) == T.AMBIGUOUS]
    assert len(payloads) >= 4
    outcomes = set()
    for mb, (ew, ns) in itertools.product(payloads, REF_VECTORS):
        for S in (40, 2000):                                  # S = 2000: the track alone decides the 5,0 reading
            outcomes.add(both_ways(mb, K.ground_frame(K.A, ew, ns, vr=0), max_speed_diff_kt=S))
    assert outcomes >= {SETTLED_50, STAYS}
    # the track check's own limit: distance 1 passes, 2 fails (BOTH's sector 11 against sectors 12, 13, 10 and 9)
    for (ew, ns), sector, want in (((-985, 408), 12, SETTLED_50), ((-985, 409), 13, STAYS), ((-985, -408), 11, SETTLED_50),
                                   ((-985, -985), 10, SETTLED_50), ((-984, -985), 9, STAYS)):
        assert T.sector16(ew, ns) == sector
        assert both_ways(K.BOTH, K.ground_frame(K.A, ew, ns, vr=0), max_speed_diff_kt=2000) == want, (ew, ns)


def test_heading_sector_distance_two():
    # 6,0's heading against a ground vector: distance 2 passes, 3 fails.  The heading 2040 is sector 15; the payload's
    # Mach field is 5,0's ground speed of 200 kt, which every one of these references contradicts
    mb = CM.mb_60(heading=-8, mach=100, baro=10, inertial=10)
    rec = stateless(mb)[1]
    assert int(rec["state"]) == T.AMBIGUOUS and int(rec["candidates"]) == T.C50 | T.C60
    near = dict(vr=320)
    for (ew, ns), d in (((100, 300), 1), ((300, 301), 2), ((301, 300), 3), ((-300, 301), 1), ((-301, 300), 2),
                        ((-985, 407), 3)):
        assert T.circular(15, T.sector16(ew, ns), 16) == d, (ew, ns)
        assert both_ways(mb, K.ground_frame(K.A, ew, ns, **near)) == (SETTLED_60 if d <= 2 else STAYS), (ew, ns)


def test_age():
    ref = K.ground_frame(K.A, vr=0, **{k: v for k, v in K.AGREES.items() if k != "vr"})
    beyond = math.nextafter(10.0, math.inf)
    for t, ref_time, want in ((10.0, 0.0, SETTLED_50), (beyond, 0.0, STAYS), (0.0, 0.0, SETTLED_50),
                              (-math.nextafter(0.0, 1.0), 0.0, STAYS), (5.0, 6.0, STAYS), (math.nan, 0.0, STAYS),
                              (1.0, math.nan, STAYS), (1e6 + 10.0, 1e6, SETTLED_50), (math.inf, 0.0, STAYS)):
        assert both_ways(K.BOTH, ref, t=t, ref_time=ref_time) == want, (t, ref_time)
    assert both_ways(K.BOTH, ref, t=0.5, max_age_s=0.5) == SETTLED_50
    assert both_ways(K.BOTH, ref, t=0.5, max_age_s=0.0) == STAYS
    assert both_ways(K.BOTH, ref, t=3.0, ref_time=3.0, max_age_s=0.0) == SETTLED_50
    assert both_ways(K.BOTH, None) == STAYS


def test_every_subtype_with_and_without_each_flag():
    outcomes = set()
    refs = []
    for st in (1, 2):
        for speed, vr in itertools.product((False, True), (None, 0, 5760, -640)):
            raw = dict(dew=1, vew=104 if st == 2 else 414, dns=1, vns=31 if st == 2 else 121) if speed else {}
            if vr is not None:
                raw.update(svr=int(vr < 0), vr=abs(vr) // 64 + 1)
            refs.append(K.vel_frame(K.A, st, **raw))
    for st in (3, 4):
        for heading, airspeed, tas, vr in itertools.product((None, 60, 1020), (None, 360, 20), (0, 1), (None, 0, 320)):
            refs.append(K.air_frame(K.A, heading=heading, airspeed=airspeed, tas=tas, vr=vr, st=st))
    refs += [K.vel_frame(K.A, st, dew=1, vew=414, dns=1, vns=121) for st in (0, 5, 6, 7)]          # no velocity message
    for mb, ref in itertools.product((K.BOTH, HEAD_EVEN, HEAD_ODD), refs):
        outcomes.add(both_ways(mb, ref))
    assert outcomes == {SETTLED_50, SETTLED_60, STAYS}


def test_other_candidate_sets_and_states_stay():
    ref = K.ground_frame(K.A, **K.AGREES)
    _, fr, claim = CK.ambiguous()
    n = 0
    for j, (_, c) in enumerate(claim[1]):
        msg = fr["bytes"][j].tobytes()
        rec = CM.commb([msg])["recs"][0]
        got = A.host_commb_settle(msg, rec, A.host_commb_reference(ref), 1.0)
        if c != T.C50 | T.C60:
            n += 1
            assert got.tobytes() == rec.tobytes()
    assert n >= 3
    for k in CK.KNOWN_FRAMES:                                                   # ONE records, and NOT_COMMB
        for msg in (bytes(k), bytes([17 << 3]) + bytes(k)[1:]):
            rec = CM.commb([msg])["recs"][0]
            assert A.host_commb_settle(msg, rec, A.host_commb_reference(ref), 1.0).tobytes() == rec.tobytes()


def test_supported_against_merely_uncheckable_stays():
    # ST 3 with a true airspeed only: 5,0's airspeed check passes, no check applies to the 6,0 reading
    assert both_ways(K.BOTH, K.air_frame(K.A, airspeed=360, tas=1)) == STAYS
    # and the other way round: 6,0's heading passes, nothing applies to 5,0
    assert both_ways(HEAD_EVEN, K.air_frame(K.A, heading=1020)) == STAYS
    # one more check that fails on the other side settles it
    assert both_ways(K.BOTH, K.air_frame(K.A, airspeed=360, tas=1, vr=0)) == SETTLED_50


# ---- the combine --------------------------------------------------------------------------------------------------------
def parts_of(case):
    out, _, _ = K.run_model(case)
    keep = [j for j in range(len(out)) if int(out["state"][j]) != T.NOT_COMMB]
    times = [float(int(case["frames"]["offset"][j])) * K.SPS for j in keep]
    return [(out[j], t) for j, t in zip(keep, times)]


def test_contribution_and_merge_in_both_groupings():
    items = parts_of(K.registers())[:18] + parts_of(K.twelve())
    lib = [A.host_track_commb_of(r, t) for r, t in items]
    for (r, t), one in zip(items, lib):
        assert one.tobytes() == T.record(T.count(T.empty(), r, t)).tobytes(), (r, one)
    empty = A.host_track_commb_of(np.zeros(1, dtype=A.COMMB_DTYPE)[0], 3.0)
    assert empty.tobytes() == T.record(T.empty()).tobytes()
    model = T.empty()
    for r, t in items:
        T.count(model, r, t)
    left = empty
    for one in lib:
        left = A.host_track_commb_merge(left, one)
    right = empty
    for one in reversed(lib):
        right = A.host_track_commb_merge(one, right)
    assert left.tobytes() == right.tobytes() == T.record(model).tobytes()
    for a, b, c in itertools.product(lib[::3], lib[1::4], lib[2::5]):
        ab_c = A.host_track_commb_merge(A.host_track_commb_merge(a, b), c)
        a_bc = A.host_track_commb_merge(a, A.host_track_commb_merge(b, c))
        assert ab_c.tobytes() == a_bc.tobytes()
        want = T.merge(T.merge(T.as_dict(a.view(T.MODEL_DTYPE)), T.as_dict(b.view(T.MODEL_DTYPE))),
                       T.as_dict(c.view(T.MODEL_DTYPE)))
        assert ab_c.tobytes() == T.record(want).tobytes()
    for one in lib:                                                              # the identity, on both sides
        assert A.host_track_commb_merge(empty, one).tobytes() == one.tobytes()
        assert A.host_track_commb_merge(one, empty).tobytes() == one.tobytes()


@pytest.mark.parametrize("start", [U32 - 2, U32 - 1, U32])
def test_counts_saturate(start):
    settled = parts_of(K.twelve())[1]
    assert int(settled[0]["state"]) == T.SETTLED
    none = (CM.commb([K.reply(b"\xff" * 7)])["recs"][0], 2.0)
    amb = (CM.commb([K.reply(K.BOTH)])["recs"][0], 3.0)
    model = T.empty()
    for k in T.COUNTS:
        model[k] = start
    lib = np.array(T.record(model)).view(A.AIRCRAFT_COMMB_DTYPE).reshape(1)[0]
    for r, t in (settled, none, amb, settled):
        T.count(model, r, t)
        lib = A.host_track_commb_merge(lib, A.host_track_commb_of(r, t))
        assert lib.tobytes() == T.record(model).tobytes()
    assert model["n_commb"] == U32 and model["n_settled"] == min(start + 2, U32)
    two = A.host_track_commb_merge(A.host_track_commb_of(*settled), A.host_track_commb_of(*settled))
    big = np.array(T.record(dict(T.empty(), n_commb=start, n_settled=start))).view(A.AIRCRAFT_COMMB_DTYPE).reshape(1)[0]
    assert int(A.host_track_commb_merge(big, two)["n_settled"]) == min(start + 2, U32)
