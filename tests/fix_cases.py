"""Planted cases for the single-message position decode (air_rs_amd/csrc/adsb_fix.h, fix_decode) and a reference that does
not share its formula (tests/test_fix_cases.py checks the builders, the CPU mirror and the model on the CPU;
tests/test_gpu_fix_edges.py runs every case on the device).

tests/fix_model.py restates the decode in f64 with the same acos expression for NL, so it cannot tell a wrong formula
from a right one.  The reference here is EXACT: the header's formulas in fractions.Fraction on the exact values of the
site's doubles, NL from the table of DO-260's 58 transition latitudes (50 digits), range and bearing from mpmath at 50
digits.  Where the decode's floor(0.5 + mod(s, d) / d - y) sits on (or within 2^-30 of) an integer, the two candidate
positions half a zone either side of the site are equally near and rounding decides between them: such a case is a TIE,
and is compared for equality between implementations only.  (2^-30: the f64 evaluation of the argument, a value below
64, is off by a few times 1e-14 at the most; tests/test_fix_cases.py asserts that no planted argument that is not meant as
a tie lies within 2^-24 of an integer, a million times the f64 error.)

A case is (site, frame, class name, expected verdict, tag): site = (latitude, longitude, max_range_nm), the verdict is what
the BUILDER means the case to be, and test_fix_cases.py holds every one of them against the exact reference.  Every frame
has an ICAO of its own and a correct CRC."""
import math
from collections import namedtuple
from fractions import Fraction as Fr
from functools import lru_cache

import mpmath
import numpy as np

from tests import fix_model as M

Case = namedtuple("Case", "site frame cls verdict tag")
Position = namedtuple("Position", "lat lon tie nl margin")    # lon None: |lat| > 90; margin: see exact_position
ACCEPTED, REJECTED, NONE = "accepted", "rejected", "none"
CLASSES = ("nl", "special", "site_edges", "southwest", "meridian", "half_zone", "range_bearing", "fields")
MAX_CASES, MAX_SITES = 16384, 256
TIE_WITHIN = Fr(1, 1 << 30)
R_NM = Fr(3440065, 1000)
HALF = Fr(1, 2)
GRID = 1 << 17
MIN_SUBNORMAL = -5e-324

_mp = mpmath.mp.clone()
_mp.dps = 50

# the header's movement table, written out: MOVEMENT_KT[m] for m = 0..127, None where the field carries no speed
MOVEMENT_KT = [
    None, 0.0, 0.125, 0.25, 0.375, 0.5, 0.625, 0.75, 0.875, 1.0, 1.25, 1.5, 1.75,
    2.0, 2.5, 3.0, 3.5, 4.0, 4.5, 5.0, 5.5, 6.0, 6.5, 7.0, 7.5, 8.0, 8.5, 9.0, 9.5, 10.0, 10.5, 11.0, 11.5, 12.0, 12.5,
    13.0, 13.5, 14.0, 14.5,
    15.0, 16.0, 17.0, 18.0, 19.0, 20.0, 21.0, 22.0, 23.0, 24.0, 25.0, 26.0, 27.0, 28.0, 29.0, 30.0, 31.0, 32.0, 33.0, 34.0,
    35.0, 36.0, 37.0, 38.0, 39.0, 40.0, 41.0, 42.0, 43.0, 44.0, 45.0, 46.0, 47.0, 48.0, 49.0, 50.0, 51.0, 52.0, 53.0, 54.0,
    55.0, 56.0, 57.0, 58.0, 59.0, 60.0, 61.0, 62.0, 63.0, 64.0, 65.0, 66.0, 67.0, 68.0, 69.0,
    70.0, 72.0, 74.0, 76.0, 78.0, 80.0, 82.0, 84.0, 86.0, 88.0, 90.0, 92.0, 94.0, 96.0, 98.0,
    100.0, 105.0, 110.0, 115.0, 120.0, 125.0, 130.0, 135.0, 140.0, 145.0, 150.0, 155.0, 160.0, 165.0, 170.0,
    175.0, None, None, None]
assert len(MOVEMENT_KT) == 128


# ---- the exact reference ------------------------------------------------------------------------------------------------
def _mpf(v):
    """An int, a float (exactly) or a Fraction as a 50-digit mpf."""
    if isinstance(v, Fr):
        return _mp.mpf(v.numerator) / _mp.mpf(v.denominator)
    return _mp.mpf(v)


@lru_cache(maxsize=None)
def transitions():
    """{NL: lat_NL in degrees (mpf)} for NL 2..59, DO-260's table: a latitude has NL zones if lat_(NL+1) <= |lat| < lat_NL.
    lat_2 is acos(sin 3 degrees) = 87 exactly."""
    out = {2: _mp.mpf(87)}
    for nl in range(3, 60):
        c = (1 - _mp.cos(_mp.pi / 30)) / (1 - _mp.cos(2 * _mp.pi / nl))
        out[nl] = _mp.degrees(_mp.acos(_mp.sqrt(c)))
    assert all(out[nl] < out[nl - 1] for nl in range(3, 60)) and 10.47 < out[59] < 10.48
    return out


def exact_nl(lat):
    """NL of an exact latitude (a Fraction); 87 exactly has 2 zones, as the reference's calc_num_zones says."""
    a = abs(lat)
    if a > 87:
        return 1
    if a == 87:
        return 2
    a = _mpf(a)
    for nl in range(59, 1, -1):
        if a < transitions()[nl]:
            return nl
    raise AssertionError(lat)


def spans(odd, surface):
    """(span, dLat) as Fractions"""
    span = Fr(90 if surface else 360)
    return span, span / (60 - odd)


def _floor_mod(a, b):
    return a - b * math.floor(a / b)


def _to_integer(u):
    return abs(u - math.floor(u + HALF))


def exact_position(site, odd, surface, lat_cpr, lon_cpr, bias=(0, 0)):
    """The header's decode in exact arithmetic -> Position(lat, lon in [-180, 180], tie, NL, margin).  margin: how far
    the nearer of the two floor arguments (latitude's, longitude's) is from an integer; tie: margin <= 2^-30.  bias: added
    to the two arguments before the floor: +-2^-20 gives the two candidates of a tie."""
    span, d_lat = spans(odd, surface)
    s_lat, s_lon = Fr(site[0]), Fr(site[1])
    y, x = Fr(lat_cpr, GRID), Fr(lon_cpr, GRID)
    u = HALF + _floor_mod(s_lat, d_lat) / d_lat - y
    lat = d_lat * (math.floor(s_lat / d_lat) + math.floor(u + bias[0]) + y)
    margin = _to_integer(u)
    if abs(lat) > 90:
        return Position(lat, None, margin <= TIE_WITHIN, None, margin)
    nl = exact_nl(lat)
    d_lon = span / max(nl - odd, 1)
    v = HALF + _floor_mod(s_lon, d_lon) / d_lon - x
    lon = d_lon * (math.floor(s_lon / d_lon) + math.floor(v + bias[1]) + x)
    while lon < -180:
        lon += 360
    while lon > 180:
        lon -= 360
    margin = min(margin, _to_integer(v))
    return Position(lat, lon, margin <= TIE_WITHIN, nl, margin)


def exact_range_bearing(site, lat, lon):
    """(haversine range in NM, initial bearing in degrees in [0, 360)) of the header's spherical formulas at 50 digits"""
    mp = _mp
    p1, p2 = mp.radians(_mpf(site[0])), mp.radians(_mpf(lat))
    dl = mp.radians(_mpf(lon) - _mpf(site[1]))
    h = mp.sin((p2 - p1) / 2) ** 2 + mp.cos(p1) * mp.cos(p2) * mp.sin(dl / 2) ** 2
    rng = 2 * _mpf(R_NM) * mp.asin(min(mp.mpf(1), mp.sqrt(h)))
    brg = mp.degrees(mp.atan2(mp.sin(dl) * mp.cos(p2), mp.cos(p1) * mp.sin(p2) - mp.sin(p1) * mp.cos(p2) * mp.cos(dl)))
    if brg < 0:
        brg += 360
    return rng, brg


def frame_fields(frame):
    """(df, tc, odd, lat_cpr, lon_cpr, bits) of a frame"""
    f = M.bits(frame)
    return bytes(frame)[0] >> 3, f(0, 5), f(21, 1), f(22, 17), f(39, 17), f


def exact_decode(site, frame, bias=(0, 0)):
    """What the header says of one frame against one site, from the exact position: a dict with verdict, flags, tie and,
    accepted, lat / lon (Fractions), range / bearing (mpf), altitude, ground_speed_kt, track_deg, type_code, cpr_odd.
    A rejected frame keeps its range (inf for |lat| > 90)."""
    df, tc, odd, lat_cpr, lon_cpr, f = frame_fields(frame)
    surface = 5 <= tc <= 8
    if df != 17 or not (surface or 9 <= tc <= 18 or 20 <= tc <= 22):
        return {"verdict": NONE, "flags": 0, "tie": False}
    kind = M.SURFACE if surface else 0
    pos = exact_position(site, odd, surface, lat_cpr, lon_cpr, bias)
    out = {"verdict": REJECTED, "flags": M.REJECTED | kind, "tie": pos.tie, "range": _mp.inf, "position": pos}
    if pos.lon is None:
        return out
    rng, brg = exact_range_bearing(site, pos.lat, pos.lon)
    out["range"] = rng
    if rng > _mpf(min(site[2], 45.0) if surface else site[2]):
        return out
    out.update(verdict=ACCEPTED, flags=M.VALID | kind, lat=pos.lat, lon=pos.lon, bearing=brg, altitude=0,
               ground_speed_kt=0.0, track_deg=0.0, type_code=tc, cpr_odd=odd)
    if surface:
        if MOVEMENT_KT[f(5, 7)] is not None:
            out["ground_speed_kt"] = MOVEMENT_KT[f(5, 7)]
            out["flags"] |= M.SPEED
        if f(12, 1):
            out["track_deg"] = f(13, 7) * 2.8125
            out["flags"] |= M.TRACK
    elif tc <= 18:
        code = f(8, 12)                                                 # seven bits, the Q bit, four bits
        out["altitude"] = ((code >> 5) << 4 | (code & 0xF)) * (25 if code & 0x10 else 100) - 1000
        out["flags"] |= M.ALT
    return out


# ---- the grid: a position a message can say is (dLat k / 2^17, dLon q / 2^17) for integers k, q ---------------------------
def grid_lat(k, odd, surface):
    return spans(odd, surface)[1] * k / GRID


def lat_index(lat, odd, surface):
    """The grid latitude nearest `lat` (DO-260's encoder: floor(2^17 lat / dLat + 1/2))"""
    return math.floor(Fr(lat) * GRID / spans(odd, surface)[1] + HALF)


def lon_step(k, odd, surface):
    """dLon / 2^17 at the grid latitude k"""
    span, _ = spans(odd, surface)
    return span / max(exact_nl(grid_lat(k, odd, surface)) - odd, 1) / GRID


def lon_index(lon, k, odd, surface):
    return math.floor(Fr(lon) / lon_step(k, odd, surface) + HALF)


class _Builder:
    def __init__(self, oracle, first_icao):
        self.oracle, self.icao, self.out = oracle, first_icao, []

    def next_icao(self):
        self.icao += 1
        return self.icao

    def add(self, site, cls, verdict, odd, surface, k, lon=None, q=None, tag="", tc=None, **kw):
        """The message of format (odd, surface) that says grid latitude k and grid longitude q (or the one nearest
        `lon`; where |lat| > 90 there is no NL and lon_cpr is 12345)."""
        n = len(self.out)
        if tc is None:
            tc = 5 + n % 4 if surface else (9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 20, 21, 22)[n % 13]
        if abs(grid_lat(k, odd, surface)) > 90:
            q = 12345
        elif q is None:
            q = lon_index(lon, k, odd, surface)
        frame = M.position_frame(self.oracle, self.next_icao(), tc, odd, k % GRID, q % GRID, **kw)
        self.out.append(Case(tuple(float(v) for v in site), frame, cls, verdict, tag))

    def add_at(self, site, cls, verdict, odd, surface, lat, lon, **kw):
        """... that says the grid position nearest (lat, lon)"""
        self.add(site, cls, verdict, odd, surface, lat_index(lat, odd, surface), lon=lon, **kw)


FORMATS = ((0, 0), (1, 0), (0, 1), (1, 1))               # (odd, surface)


def _nl(b):
    """Every NL transition, both hemispheres, all four formats: the two grid latitudes below it and the two above, at a
    site a quarter of a degree equatorward on the meridian the message names.  1,856 cases, 116 sites, all accepted."""
    for nl in range(2, 60):
        t = transitions()[nl]
        for south in (0, 1):
            sign = -1 if south else 1
            lon = (100.37 + 1.3 * nl) * (1 if (nl + south) % 2 else -1)          # 102.97 .. 177.07, east and west
            site = (sign * (round(float(t), 2) - 0.25), lon, 180.0)
            for odd, surface in FORMATS:
                k0 = int(_mp.floor(t * GRID / _mpf(spans(odd, surface)[1])))     # the last grid latitude with NL zones
                for dk in (-1, 0, 1, 2):
                    b.add(site, "nl", ACCEPTED, odd, surface, sign * (k0 + dk), lon=lon, tag=f"NL {nl}")


def _special(b):
    def k_of(deg, odd, surface):
        k = Fr(deg) * GRID / spans(odd, surface)[1]
        assert k.denominator == 1, (deg, odd, surface)
        return int(k)
    # lat exactly 0, +-87: even airborne y = 1/2 with j = 14 / -15, even surface y = 0 with j = +-58
    for surface in (0, 1):
        for deg, site in ((87, (86.8, 100.5)), (-87, (-86.8, -100.5)), (0, (0.2, -100.25)), (0, (-0.2, 100.25))):
            b.add(site + (180.0,), "special", ACCEPTED, 0, surface, k_of(deg, 0, surface), lon=site[1], tag=f"lat {deg}")
    # lat exactly +-90 (every format reaches it), accepted; one CPR step beyond, rejected
    for odd, surface in FORMATS:
        for sign in (1, -1):
            k = sign * k_of(90, odd, surface)
            b.add((sign * 89.6, sign * -120.0, 180.0), "special", ACCEPTED, odd, surface, k, lon=sign * -120.0, tag="pole")
            b.add((sign * 89.9, sign * 33.0, 180.0), "special", REJECTED, odd, surface, k + sign, tag="beyond")
    # 87 < |lat| < 90: one zone, dLon = span; sites above 87, one of them beside the antimeridian
    for site in ((88.0, 170.0), (-88.5, -175.0), (87.5, 10.0)):
        for odd, surface in FORMATS:
            for d_lat, d_lon in ((0.2, 15.0), (0.3, -15.0), (-0.2, 4.0)):
                lat = site[0] + math.copysign(d_lat, site[0] * d_lat)            # +: poleward
                b.add_at(site + (180.0,), "special", ACCEPTED, odd, surface, lat, site[1] + d_lon, tag="one zone")
    # NL 2 (86.54 .. 87) with the odd format: max(NL - 1, 1) zones
    for site in ((86.7, 140.0), (-86.7, -40.0)):
        for surface in (0, 1):
            b.add_at(site + (180.0,), "special", ACCEPTED, 1, surface, math.copysign(86.8, site[0]), site[1] + 5.0,
                     tag="NL 2 odd")


SITE_EDGE_LATS = (48.0, 12.0, 0.0, -0.0, MIN_SUBNORMAL, 90.0, -90.0)
SITE_EDGE_LONS = (0.0, -0.0, MIN_SUBNORMAL, 180.0, -180.0)


def _site_edges(b):
    """Sites on exact multiples of dLat (6, 1.5; of every dLat: 0) and of dLon: the messages that say the grid point
    nearest the site and the eight around it, one CPR step away."""
    for s_lat in SITE_EDGE_LATS:
        for s_lon in SITE_EDGE_LONS:
            for odd, surface in FORMATS:
                k0 = lat_index(s_lat, odd, surface)
                for dk in (-1, 0, 1):
                    k = k0 + dk
                    beyond = abs(grid_lat(k, odd, surface)) > 90
                    q0 = 0 if beyond else lon_index(s_lon, k, odd, surface)
                    for dq in (-1, 0, 1):
                        b.add((s_lat, s_lon, 180.0), "site_edges", REJECTED if beyond else ACCEPTED, odd, surface, k,
                              q=q0 + dq, tag=f"{dk:+d} {dq:+d}")


def _southwest(b):
    offsets = ((-1.0, -1.5), (1.0, 1.5), (-0.4, 0.6), (0.5, -0.7), (-0.01, -0.01))
    for site in ((-33.9, -58.4), (-0.1, -0.1), (0.1, 0.1), (-45.7, -170.2)):
        for odd, surface in FORMATS:
            scale = 0.3 if surface else 1.0
            for d_lat, d_lon in offsets:
                b.add_at(site + (180.0,), "southwest", ACCEPTED, odd, surface, site[0] + scale * d_lat,
                         site[1] + scale * d_lon)


def band_latitude(nl):
    """A latitude (two decimals) in the middle of the band with NL zones"""
    t = transitions()
    lat = round(float((t[nl + 1] + t[nl]) / 2), 2)
    assert exact_nl(Fr(lat)) == nl
    return lat


def _meridian(b):
    """Sites at +-179.99 and +-180.0, targets 1, 300 and 5000 CPR steps either side of the antimeridian; where the zone
    count makes dLon a binary fraction of a degree (36 zones: 10 or 2.5 degrees) also the grid point ON it, which the
    decode must leave at +180 from the east and at -180 from the west."""
    for s_lat in (band_latitude(36), -band_latitude(37), 10.0, -35.0):
        for s_lon in (179.99, -179.99, 180.0, -180.0):
            for odd, surface in FORMATS:
                k = lat_index(s_lat, odd, surface)
                step = lon_step(k, odd, surface)
                zones = spans(odd, surface)[0] / (step * GRID)
                at_180 = Fr(180) / step
                assert at_180.denominator == 1
                offsets = (-5000, -300, -1, 1, 300, 5000) + ((0,) if zones == 36 else ())
                for dq in offsets:
                    b.add((s_lat, s_lon, 180.0), "meridian", ACCEPTED, odd, surface, k,
                          q=int(math.copysign(at_180, s_lon)) + dq, tag=f"{dq:+d}")


def _half_zone(b):
    def either_side(edge, step):
        """(the grid index just short of `edge`, the one just past it), `edge` in the direction of `step` (+-1)"""
        h = edge
        if step > 0:
            return math.ceil(h) - 1, math.floor(h) + 1
        return math.floor(h) + 1, math.ceil(h) - 1

    for s_lat, s_lon in ((40.0, -100.0), (-20.0, 30.0)):
        for surface in (0, 1):
            limits = (30.0, 45.0, 180.0) if surface else (180.0,)
            for limit in limits:
                site = (s_lat, s_lon, limit)
                for odd in (0, 1):
                    # inside the limits: accepted (a surface message only where the site's own limit allows it)
                    for dist in ((29.9, 44.9) if surface else (179.9,)):
                        for brg in (0.0, 90.0, 180.0, 270.0):
                            lat, lon = M.destination(site, dist, brg)
                            b.add_at(site, "half_zone", ACCEPTED if dist < limit else REJECTED, odd, surface, lat, lon,
                                     tag=f"{dist} NM")
                    # one CPR step short of half a zone and one past it: the decode is right, then wrong, and both lie
                    # beyond the range limit
                    _, d_lat = spans(odd, surface)
                    for sign in (1, -1):
                        edge = (Fr(s_lat) + sign * d_lat / 2) * GRID / d_lat
                        for k, tag in zip(either_side(edge, sign), ("short of half dLat", "past half dLat")):
                            b.add(site, "half_zone", REJECTED, odd, surface, k, lon=s_lon, tag=tag)
                    k = lat_index(s_lat, odd, surface)
                    step = lon_step(k, odd, surface)
                    for sign in (1, -1):
                        edge = (Fr(s_lon) + sign * step * GRID / 2) / step
                        for q, tag in zip(either_side(edge, sign), ("short of half dLon", "past half dLon")):
                            b.add(site, "half_zone", REJECTED, odd, surface, k, q=q, tag=tag)
    # exact ties: the site half a zone from the grid point named.  6 and 1.5 degrees of latitude; 10 degrees of longitude
    # (36 zones) and 360 (one zone); and the site a subnormal south of the equator, where mod(s, d) / d rounds to 1 or 0
    lat36 = band_latitude(36)
    k36 = lat_index(lat36, 0, 0)
    for site, odd, surface, k, q in (((45.0, 8.0), 0, 0, 8 * GRID, None), ((45.0, 8.0), 0, 1, 30 * GRID + GRID // 2, None),
                                     ((MIN_SUBNORMAL, 10.0), 0, 0, GRID // 2, None),
                                     ((MIN_SUBNORMAL, 10.0), 0, 1, GRID // 2, None),
                                     ((lat36, 5.0), 0, 0, k36, 0), ((lat36, -5.0), 0, 0, k36, 0),
                                     ((88.0, 180.0), 0, 0, lat_index(88.0, 0, 0), 0),
                                     ((88.0, -180.0), 1, 0, lat_index(88.0, 1, 0), 0),
                                     ((10.0, MIN_SUBNORMAL), 0, 0, lat_index(10.0, 0, 0), GRID // 2)):
        b.add(site + (180.0,), "half_zone", REJECTED, odd, surface, k, lon=site[1], q=q, tag="tie")


HAIR_WEST = dict(first_site=(47.45, 8.56), odd=0, lat_cpr=70000, lon_cpr=30000, tc=11, south=0.5)


def hair_west_site(east):
    """The site of the issue's reproduction: half a degree south and `east` degrees east of where the HAIR_WEST message
    decodes to against (47.45, 8.56)."""
    p = exact_position(HAIR_WEST["first_site"], 0, 0, HAIR_WEST["lat_cpr"], HAIR_WEST["lon_cpr"])
    return (float(p.lat) - HAIR_WEST["south"], float(p.lon) + east, 180.0)


def _range_bearing(b):
    # the site exactly on a grid point whose coordinates are doubles: dLat 6 or 1.5, dLon 10 or 2.5 (36 zones)
    for surface in (0, 1):
        k = lat_index(band_latitude(36), 0, surface)
        q = 5 * GRID // 4 + 40000
        site = (float(grid_lat(k, 0, surface)), float(lon_step(k, 0, surface) * q), 180.0)
        assert Fr(site[0]) == grid_lat(k, 0, surface) and Fr(site[1]) == lon_step(k, 0, surface) * q
        b.add(site, "range_bearing", ACCEPTED, 0, surface, k, q=q, tag="on the site")
    # due north and south on the prime meridian (on every format's grid), due east and west along the equator
    for odd, surface in FORMATS:
        d = 0.3 if surface else 1.0
        for s_lat in (30.0, -30.0):
            for sign, tag in ((1, "bearing 0"), (-1, "bearing 180")):
                b.add((s_lat, 0.0, 180.0), "range_bearing", ACCEPTED, odd, surface, lat_index(s_lat + sign * d, odd, surface),
                      q=0, tag=tag)
        for s_lon in (20.0, -160.0):
            for sign, tag in ((1, "bearing 90"), (-1, "bearing 270")):
                b.add((0.0, s_lon, 180.0), "range_bearing", ACCEPTED, odd, surface, 0, lon=s_lon + sign * d, tag=tag)
    # a hair west of due north: the f64 bearing is below 360 and its one rounding to f32 is not
    for east, tag in ((1e-7, "hair west"), (1e-6, "a little west")):
        b.add(hair_west_site(east), "range_bearing", ACCEPTED, 0, 0, HAIR_WEST["lat_cpr"], q=HAIR_WEST["lon_cpr"], tag=tag,
              tc=HAIR_WEST["tc"])
    # ranges within 1e-3 NM of a limit and no closer than 1e-6 NM.  The site's own limit is a free double:
    for surface, d in ((0, 2.0), (1, 0.3)):
        k = lat_index(40.0 + d, 0, surface)
        q = lon_index(-100.0, k, 0, surface)
        rng = float(exact_range_bearing((40.0, -100.0), grid_lat(k, 0, surface), lon_step(k, 0, surface) * q)[0])
        for gap in (2e-6, 5e-4, -2e-6, -5e-4):
            b.add((40.0, -100.0, rng + gap), "range_bearing", ACCEPTED if gap > 0 else REJECTED, 0, surface, k, q=q,
                  tag="limit")
    # ... the caps are not.  Surface, 45 NM: the grid latitudes due north of the site pass it in steps of 6.9e-4 NM
    step_nm = float(_mpf(R_NM) * _mp.radians(_mpf(grid_lat(1, 0, 1))))
    k0 = lat_index(40.0, 0, 1)
    found = {}
    for dk in range(int(45.0 / step_nm) - 3, int(45.0 / step_nm) + 4):
        gap = float(exact_range_bearing((40.0, 0.0), grid_lat(k0 + dk, 0, 1), 0)[0] - 45)
        if 1e-6 < abs(gap) < 1e-3:
            found.setdefault(gap > 0, k0 + dk)
    assert set(found) == {False, True}
    for limit in (45.0, 180.0):
        for past, k in found.items():
            b.add((40.0, 0.0, limit), "range_bearing", REJECTED if past else ACCEPTED, 0, 1, k, q=0, tag="limit")
    # airborne, 180 NM: the site is placed on the target's meridian, 180 -+ 5e-4 NM of arc to the south
    k = lat_index(43.0, 0, 0)
    for gap in (-5e-4, 5e-4):
        arc = _mp.degrees((180 + _mpf(gap)) / _mpf(R_NM))
        b.add((float(_mpf(grid_lat(k, 0, 0)) - arc), 0.0, 180.0), "range_bearing", ACCEPTED if gap < 0 else REJECTED, 0, 0, k,
              q=0, tag="limit")


FIELD_SITES = tuple((47.45 + i, 8.56, 180.0) for i in range(4))


def _fields(b):
    """Every movement value with and without a track, every altitude code, DF 16 / 17 / 18 x nine type codes: each
    message says (the grid point nearest) its site's own position."""
    site = FIELD_SITES[0]
    for m in range(128):
        for valid in (0, 1):
            b.add_at(site, "fields", ACCEPTED, m & 1, 1, site[0], site[1], tag=f"movement {m}", tc=5 + m % 4, movement=m,
                     track_valid=valid, track=(37 * m + 5) % 128)
    for code in range(4096):
        site = FIELD_SITES[code >> 10]
        b.add_at(site, "fields", ACCEPTED, code & 1, 0, site[0], site[1], tag="altitude", tc=9 + code % 10, alt_code=code)
    site = FIELD_SITES[0]
    for df in (16, 17, 18):
        for tc in (4, 5, 8, 9, 18, 19, 20, 22, 23):
            surface = int(5 <= tc <= 8)
            k = lat_index(site[0], 1, surface)
            me = tc << 51 | 1 << 34 | (k % GRID) << 17 | lon_index(site[1], k, 1, surface) % GRID
            position = df == 17 and tc not in (4, 19, 23)
            b.out.append(Case(site, M.raw_frame(b.oracle, b.next_icao(), me, df=df), "fields",
                              ACCEPTED if position else NONE, f"DF {df} TC {tc}"))


BUILDERS = dict(nl=_nl, special=_special, site_edges=_site_edges, southwest=_southwest, meridian=_meridian,
                half_zone=_half_zone, range_bearing=_range_bearing, fields=_fields)
_cache = {}


def cases(oracle):
    """Every case, class by class in CLASSES order (built once per process)."""
    if "cases" not in _cache:
        b = _Builder(oracle, 0x100000)
        for cls in CLASSES:
            BUILDERS[cls](b)
        _cache["cases"] = tuple(b.out)
    return _cache["cases"]


def reference(oracle):
    """exact_decode of every case, aligned with cases() (computed once per process and not to be changed)."""
    if "reference" not in _cache:
        _cache["reference"] = tuple(exact_decode(c.site, c.frame) for c in cases(oracle))
    return _cache["reference"]


def sites_of(all_cases):
    """The distinct sites in order of first use, and each case's index into them.  -0.0 and 0.0 are different sites."""
    index, sites, where = {}, [], []
    for c in all_cases:
        k = tuple((v, math.copysign(1.0, v)) for v in c.site)
        if k not in index:
            index[k] = len(sites)
            sites.append(c.site)
        where.append(index[k])
    return sites, where


# ---- what the checks share ----------------------------------------------------------------------------------------------
def f32_half_ulp(value):
    """Half the spacing of f32 at `value`, plus 1e-9 for the f64 evaluation before the one rounding"""
    return 0.5 * float(np.spacing(np.float32(abs(float(value))))) + 1e-9


def bearing_gap(got, want):
    d = abs(float(got) - float(want))
    return min(d, 360.0 - d)
