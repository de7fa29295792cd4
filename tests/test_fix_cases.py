"""tests/fix_cases.py on the CPU: the builders do what they say, adsb_host_fix_of and tests/fix_model.py give the exact
reference's answer on every case, and a table of deliberately wrong decodes each fails on the class planted for it.

Bounds.  Off ties, latitude and longitude lie within 1e-12 degree of the exact rational value: the decode before NL is a
handful of f64 operations on values below 180, a few ulps (2.8e-14 each) in all, and NL is an integer.  range_nm and
bearing_deg are f64 values rounded to f32 once, so they lie within half an f32 step of the 50-digit value, plus 1e-9 for
the f64 evaluation (bearing from 1 NM on, where the position's 1e-13 degree cannot turn it).  The limit is tested on
the f64 range, so an accepted frame's f32 range_nm may exceed a fractional limit by half an f32 step: that is documented
in include/adsb_hip.h and not asserted against.  Mirror and model are compared bit for bit, ties included."""
import collections
import math

import numpy as np
import pytest

from tests import fix_cases as FC
from tests import fix_model as M

Fr = FC.Fr
COUNTS = {"nl": 1856, "special": 64, "site_edges": 1260, "southwest": 80, "meridian": 400, "half_zone": 249,
          "range_bearing": 50, "fields": 4379}


@pytest.fixture(scope="module")
def cases(oracle):
    return FC.cases(oracle)


@pytest.fixture(scope="module")
def reference(oracle):
    return FC.reference(oracle)


# ---- the builders ---------------------------------------------------------------------------------------------------------
def test_builders_do_what_they_say(oracle, cases, reference):
    assert dict(collections.Counter(c.cls for c in cases)) == COUNTS and len(cases) < FC.MAX_CASES
    assert [c.cls for c in cases] == sorted((c.cls for c in cases), key=FC.CLASSES.index)
    sites, where = FC.sites_of(cases)
    assert len(sites) <= FC.MAX_SITES and all(sites[w] == c.site for w, c in zip(where, cases))
    assert all(-90 <= s[0] <= 90 and -180 <= s[1] <= 180 and 0 < s[2] <= 180 for s in sites)
    icaos = [int.from_bytes(c.frame[1:4], "big") for c in cases]
    assert len(set(icaos)) == len(cases)
    for c in cases:
        crc = oracle.get_adsb_crc(c.frame[:11])
        assert len(c.frame) == 14 and c.frame[11:] == bytes([crc >> 16 & 0xFF, crc >> 8 & 0xFF, crc & 0xFF])
    # every verdict is the exact reference's, and the ties are the cases planted as ties
    for k, (c, r) in enumerate(zip(cases, reference)):
        assert c.verdict == r["verdict"], (k, c, float(r.get("range", 0)))
        assert r["tie"] == (c.tag == "tie"), (k, c)
    assert sum(r["tie"] for r in reference) == 9
    margins = [r["position"].margin for r in reference if "position" in r and not r["tie"]]
    print(f"the floor argument nearest an integer off the ties: {float(min(margins)):.3g}")
    assert min(margins) > Fr(1, 1 << 24)
    assert collections.Counter(c.verdict for c in cases)[FC.REJECTED] > 150


def test_nl_cases_straddle_every_transition(cases, reference):
    """1,856 accepted cases; at each of the 58 x 2 x 4 transitions the four grid latitudes have NL, NL, NL - 1, NL - 1
    zones, and the one nearest its (irrational) transition is 8.1e-9 degree from it."""
    nl = [(c, r) for c, r in zip(cases, reference) if c.cls == "nl"]
    assert len(nl) == 1856 and all(r["verdict"] == FC.ACCEPTED for _, r in nl)
    assert all(abs(c.site[1]) >= 100 for c, _ in nl) and {c.site[1] > 0 for c, _ in nl} == {False, True}
    nearest = math.inf
    for at in range(0, len(nl), 4):
        n = int(nl[at][0].tag.split()[1])
        assert [r["position"].nl for _, r in nl[at:at + 4]] == [n, n, n - 1, n - 1], nl[at][0]
        for _, r in nl[at:at + 4] if n > 2 else ():               # (87 itself is a grid latitude of the even formats)
            nearest = min(nearest, abs(float(FC._mpf(abs(r["lat"])) - FC.transitions()[n])))
    print(f"the grid latitude nearest a transition: {nearest:.3g} degree")
    assert 1e-9 < nearest < 1e-8


def test_planted_edges_are_there(cases, reference):
    both = list(zip(cases, reference))
    of = lambda cls: [(c, r) for c, r in both if c.cls == cls]
    # special: lat exactly 0, +-87, +-90; one step beyond rejected for |lat| > 90; one zone; NL 2 with the odd format
    lats = collections.Counter(r["lat"] for c, r in of("special") if r["verdict"] == FC.ACCEPTED)
    assert lats[0] == 4 and lats[87] == lats[-87] == 2 and lats[90] == lats[-90] == 4
    assert sum(r["position"].lon is None for c, r in of("special")) == 8
    zones = collections.Counter((r["position"].nl, r["cpr_odd"]) for c, r in of("special") if r["verdict"] == FC.ACCEPTED)
    assert zones[(1, 0)] > 10 and zones[(1, 1)] > 10 and zones[(2, 1)] == 4 and zones[(2, 0)] == 4
    # site_edges: 35 sites, signed zeros and the subnormal among them, and the site at the pole turning a step away
    edge_sites = {(c.site[0], math.copysign(1, c.site[0]), c.site[1], math.copysign(1, c.site[1])) for c, _ in of("site_edges")}
    assert len(edge_sites) == 35
    assert sum(r["verdict"] == FC.REJECTED for c, r in of("site_edges")) == 2 * 5 * 4 * 3
    # southwest: negative sites, and targets across the equator and the prime meridian from the site
    sw = [(c, r) for c, r in of("southwest")]
    assert any(c.site[0] < 0 and c.site[1] < 0 and r["lat"] < 0 and r["lon"] < 0 for c, r in sw)
    assert any(c.site[0] < 0 < r["lat"] and c.site[1] < 0 < r["lon"] for c, r in sw)
    assert any(c.site[0] > 0 > r["lat"] and c.site[1] > 0 > r["lon"] for c, r in sw)
    # meridian: longitudes brought back from above 180 and from below -180, and +-180 themselves
    mer = of("meridian")
    assert all(r["verdict"] == FC.ACCEPTED for _, r in mer)
    assert sum(r["lon"] == 180 for _, r in mer) >= 4 and sum(r["lon"] == -180 for _, r in mer) >= 4
    assert sum(c.site[1] > 0 > r["lon"] for c, r in mer) > 50 and sum(c.site[1] < 0 < r["lon"] for c, r in mer) > 50
    # half_zone: no tie is accepted, whichever candidate is taken; the steps short of and past half a zone are rejected
    # by range, by the candidate FARTHER away in the second case (half a zone is 180.1 to 195 NM, 45.03 to 49 NM, with the
    # format and the latitude; a whole zone would be twice that)
    for c, r in of("half_zone"):
        if r["tie"]:
            for bias in ((Fr(1, 1 << 20),) * 2, (Fr(-1, 1 << 20),) * 2):
                assert FC.exact_decode(c.site, c.frame, bias)["verdict"] == FC.REJECTED, c
        if "half d" in c.tag:
            cap = 45.0 if r["flags"] & M.SURFACE else 180.0
            assert r["verdict"] == FC.REJECTED and cap < r["range"] < 1.1 * cap, (c, float(r["range"]))
    assert sum("short of" in c.tag for c, _ in of("half_zone")) == sum("past" in c.tag for c, _ in of("half_zone")) == 64
    assert sum(c.tag == "179.9 NM" and r["verdict"] == FC.ACCEPTED for c, r in of("half_zone")) == 16
    assert {(c.site[2], r["verdict"]) for c, r in of("half_zone") if c.tag == "44.9 NM"} == \
        {(30.0, FC.REJECTED), (45.0, FC.ACCEPTED), (180.0, FC.ACCEPTED)}
    # range_bearing: the limit cases lie within 1e-3 NM of their limit and no closer than 1e-6 NM
    n = 0
    for c, r in of("range_bearing"):
        if c.tag == "limit":
            limit = min(c.site[2], 45.0) if r["flags"] & M.SURFACE else c.site[2]
            assert 1e-6 < abs(float(r["range"] - FC._mpf(limit))) < 1e-3, c
            n += 1
        if c.tag.startswith("bearing"):
            assert FC.bearing_gap(r["bearing"], float(c.tag.split()[1])) < 1e-9, c
        if c.tag == "on the site":
            assert r["range"] == 0 and r["bearing"] == 0
    assert n == 14
    # no other range lies within 1e-6 NM of its limit either, so no verdict hangs on a rounding
    for c, r in both:
        if "range" in r and r["range"] != FC._mp.inf:
            limit = min(c.site[2], 45.0) if r["flags"] & M.SURFACE else c.site[2]
            assert abs(float(r["range"] - FC._mpf(limit))) > 1e-6, c
    # fields
    assert sum(c.tag == "altitude" for c, _ in of("fields")) == 4096
    assert len({r["altitude"] for c, r in of("fields") if c.tag == "altitude"}) > 2000
    assert collections.Counter(r["verdict"] for c, r in of("fields") if c.tag.startswith("DF")) == \
        {FC.ACCEPTED: 6, FC.NONE: 21}


# ---- the CPU mirror and the model -----------------------------------------------------------------------------------------
def check_against_reference(cases, reference, lat, lon, rng, brg, flags, what):
    """Arrays of one implementation, aligned with the cases, against the exact reference, ties left out -> the largest
    gaps (latitude, longitude, range, bearing).  Rejected and non-position frames carry zeros."""
    worst = [0.0, 0.0, 0.0, 0.0]
    for k, (c, r) in enumerate(zip(cases, reference)):
        if r["tie"]:
            continue
        assert int(flags[k]) == r["flags"], (what, k, c, int(flags[k]), r["flags"])
        if r["verdict"] != FC.ACCEPTED:
            assert lat[k] == 0 and lon[k] == 0 and rng[k] == 0 and brg[k] == 0, (what, k, c)
            continue
        gaps = (float(abs(Fr(float(lat[k])) - r["lat"])), float(abs(Fr(float(lon[k])) - r["lon"])),
                abs(float(rng[k]) - float(r["range"])), FC.bearing_gap(brg[k], r["bearing"]) if r["range"] >= 1 else 0.0)
        assert gaps[0] <= 1e-12 and gaps[1] <= 1e-12, (what, k, c, gaps, float(r["lat"]), float(r["lon"]))
        assert gaps[2] <= FC.f32_half_ulp(r["range"]), (what, k, c, gaps, float(r["range"]))
        assert gaps[3] <= FC.f32_half_ulp(r["bearing"]), (what, k, c, gaps, float(r["bearing"]))
        assert 0.0 <= brg[k] < 360.0, (what, k, c, brg[k])
        if c.tag == "on the site":
            assert rng[k] == 0 and brg[k] == 0, (what, k, c)
        worst = [max(a, b) for a, b in zip(worst, gaps)]
    print(f"{what}: largest gaps to the exact reference: latitude {worst[0]:.3g}, longitude {worst[1]:.3g} degree, range "
          f"{worst[2]:.3g} NM, bearing {worst[3]:.3g} degree")
    return worst


def check_fields(cases, reference, fixes, what):
    """FIX_DTYPE records of aircraft with one frame each: what the message carries beside the position."""
    for k, (c, r) in enumerate(zip(cases, reference)):
        if r["tie"]:
            continue
        a = fixes[k]
        ok = r["verdict"] == FC.ACCEPTED
        assert (int(a["n_fixes"]), int(a["n_rejected"])) == (int(ok), int(r["verdict"] == FC.REJECTED)), (what, k, c)
        want = [r[n] for n in ("ground_speed_kt", "track_deg", "altitude", "type_code", "cpr_odd", "flags")] if ok else [0] * 6
        got = [a[n] for n in ("ground_speed_kt", "track_deg", "altitude", "type_code", "cpr_odd", "flags")]
        assert got == want, (what, k, c, got, want)
        assert math.isnan(a["time"]) != ok, (what, k, c)


def mirror_records(lib, cases):
    fixes = np.zeros(len(cases), dtype=lib.FIX_DTYPE)
    flags = np.zeros(len(cases), dtype=np.uint32)
    for k, c in enumerate(cases):
        fixes[k], flags[k] = lib.host_fix_of(c.site, c.frame, 1.0 + k)
    return fixes, flags


def test_mirror_and_model_on_every_case(lib, cases, reference):
    fixes, flags = mirror_records(lib, cases)
    model = np.zeros(len(cases), dtype=M.MODEL_DTYPE)
    model_flags = np.zeros(len(cases), dtype=np.uint32)
    for k, c in enumerate(cases):
        model[k], model_flags[k] = M.fix_of(c.site, c.frame, 1.0 + k)
    # bit for bit, ties included: the 64 bytes of the record and the frame's flags
    assert np.array_equal(flags, model_flags)
    for k in range(len(cases)):
        assert fixes[k].tobytes() == model[k].tobytes(), (k, cases[k], fixes[k], model[k])
    for name, recs, fl in (("mirror", fixes, flags), ("model", model, model_flags)):
        check_against_reference(cases, reference, recs["latitude"], recs["longitude"], recs["range_nm"], recs["bearing_deg"],
                                fl, name)
        check_fields(cases, reference, recs, name)


def test_bearing_of_360_is_0(lib, oracle):
    """The known answer: a target a hair west of due north, whose f64 bearing is below 360 and rounds to 360.0f."""
    h = FC.HAIR_WEST
    frame = M.position_frame(oracle, 0x4B0360, h["tc"], h["odd"], h["lat_cpr"], h["lon_cpr"])
    first, flags = lib.host_fix_of(h["first_site"] + (180.0,), frame)
    assert flags == 5
    site = (float(first["latitude"]) - 0.5, float(first["longitude"]) + 1e-7, 180.0)
    assert np.allclose(site, FC.hair_west_site(1e-7), rtol=0, atol=1e-13)       # the case list's copy of it
    d = M.decode(site, frame)
    assert 359.99999 < d["bearing"] < 360.0 and np.float32(d["bearing"]) == np.float32(360.0)
    fix, flags = lib.host_fix_of(site, frame)
    assert flags == 5 and abs(float(fix["range_nm"]) - 30.02) < 0.005 and fix["bearing_deg"] == 0.0
    assert M.fix_of(site, frame, 0.0)[0]["bearing_deg"] == 0.0
    assert M.frame_records(site, np.array([(0, np.frombuffer(frame, dtype=np.uint8))],
                                          dtype=[("offset", "<u8"), ("bytes", "u1", (14,))]))[0]["bearing_deg"] == 0.0
    fix, flags = lib.host_fix_of((site[0], float(first["longitude"]) + 1e-6, 180.0), frame)
    assert flags == 5 and fix["bearing_deg"] == np.float32(359.99991)


# ---- mutants ----------------------------------------------------------------------------------------------------------------
def variant_position(site, odd, surface, lat_cpr, lon_cpr, nl_of=lambda lat, site: M.num_zones(lat), mod=M.mod,
                     nearest=lambda v: math.floor(0.5 + v), wrap="strict", surface_span=90.0):
    """fix_model.local_position with its decisions as arguments -> (lat, lon); lon None if |lat| > 90."""
    span = surface_span if surface else 360.0
    y, x = lat_cpr / 131072.0, lon_cpr / 131072.0
    d_lat = span / (60 - odd)
    lat = d_lat * (math.floor(site[0] / d_lat) + nearest(mod(site[0], d_lat) / d_lat - y) + y)
    if not abs(lat) <= 90.0:
        return lat, None
    d_lon = span / max(nl_of(lat, site) - odd, 1)
    lon = d_lon * (math.floor(site[1] / d_lon) + nearest(mod(site[1], d_lon) / d_lon - x) + x)
    if wrap == "strict":
        while lon < -180.0:
            lon += 360.0
        while lon > 180.0:
            lon -= 360.0
    elif wrap == "inclusive":
        while lon <= -180.0:
            lon += 360.0
        while lon >= 180.0:
            lon -= 360.0
    return lat, lon


def _polar_from_87(lat, site):
    return 1 if abs(lat) >= 87.0 else M.num_zones(lat)


# (name, the class planted for it, what is wrong)
MUTANTS = (("NL at the site's latitude", ("nl",), dict(nl_of=lambda lat, site: M.num_zones(site[0]))),
           ("NL table shifted by one step", ("nl",), dict(nl_of=lambda lat, site: max(M.num_zones(lat) - 1, 1))),
           ("fmod for floor-mod", ("southwest",), dict(mod=math.fmod)),
           ("round for floor(0.5 + .)", ("site_edges", "half_zone"),
            dict(nearest=lambda v: math.copysign(math.floor(abs(v) + 0.5), v))),
           ("no longitude wrap", ("meridian", "site_edges"), dict(wrap="none")),
           (">= / <= in the wrap", ("meridian", "site_edges"), dict(wrap="inclusive")),
           ("surface span 360", ("half_zone",), dict(surface_span=360.0)),
           ("|lat| >= 87 has one zone", ("special",), dict(nl_of=_polar_from_87)))


def position_disagreements(cases, reference, **wrong):
    """{class: cases on which the variant's position is not the reference's}: off ties the exact one within 1e-9 degree,
    on ties the model's own, bit for bit (a tie has two right answers and the implementations must give the same)."""
    out = collections.Counter()
    for c, r in zip(cases, reference):
        if r["verdict"] == FC.NONE:
            continue
        _, tc, odd, lat_cpr, lon_cpr, _ = FC.frame_fields(c.frame)
        lat, lon = variant_position(c.site, odd, int(5 <= tc <= 8), lat_cpr, lon_cpr, **wrong)
        if r["tie"]:
            want = M.local_position(c.site, odd, int(5 <= tc <= 8), lat_cpr, lon_cpr)[:2]
            same = (lat, lon) == want
        else:
            p = r["position"]
            same = abs(Fr(lat) - p.lat) <= 1e-9 and (lon is None) == (p.lon is None) and \
                (lon is None or abs(Fr(lon) - p.lon) <= 1e-9)
        if not same:
            out[c.cls] += 1
    return out


def mutant_table(cases, reference):
    """[(name, the classes planted for it, {class: disagreements})], the unchanged decode first, then the two mutants that
    are not about the position: the bearing's rounding to 360 kept, and the movement table's last piece one value short."""
    rows = [("the decode unchanged", (), position_disagreements(cases, reference))]
    rows += [(name, planted, position_disagreements(cases, reference, **wrong)) for name, planted, wrong in MUTANTS]
    kept, short = collections.Counter(), collections.Counter()
    for c, r in zip(cases, reference):
        if r["verdict"] != FC.ACCEPTED:
            continue
        d = M.decode(c.site, c.frame)
        if not np.float32(d["bearing"]) < np.float32(360.0):
            kept[c.cls] += 1
        m = FC.frame_fields(c.frame)[5](5, 7)
        if r["flags"] & M.SURFACE and (None if m >= 124 else M.movement_kt(m)) != FC.MOVEMENT_KT[m]:
            short[c.cls] += 1
    return rows + [("f32 bearing of 360 kept", ("range_bearing",), kept), ("movement 124 reserved", ("fields",), short)]


def test_mutants(cases, reference):
    rows = mutant_table(cases, reference)
    for name, planted, found in rows:
        print(f"{name:32s} planted: {', '.join(planted) or '-':22s} disagrees on: "
              + (", ".join(f"{cls} {found[cls]}" for cls in FC.CLASSES if found[cls]) or "nothing"))
    assert not rows[0][2], rows[0]
    for name, planted, found in rows[1:]:
        assert any(found[cls] for cls in planted), (name, dict(found))      # no mutant survives its class
    needed = {cls for _, planted, found in rows[1:] for cls in planted if found[cls]}
    assert needed == set(FC.CLASSES), set(FC.CLASSES) - needed               # and every class is needed by one
