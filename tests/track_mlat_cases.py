"""The cases tests/test_track_mlat_host.py walks the CPU mirror (adsb_host_track_mlat_of) and the model
(tests/track_mlat_model.py) over: (name, limit in metres, 14 frame bytes, adsb_mlat_fix record, frame time).  Every
planted disagreement is far from the limit it is judged by: honest frames lie below 50 m, displaced ones above 2 km,
against 1000 m, so DISAGREE and n_disagree are compared exactly on every case."""
import math

from tests import fix_model as F
from tests import track_mlat_model as M

LIMIT = 1000.0
GOOD = M.FIX_ATTEMPTED | 0x2 | M.FIX_VALID
# where the fixes lie: mid latitudes, the equator, both poles, the antimeridian from both sides and on it
PLACES = {"mid": (47.3, 8.5), "south": (-33.9, 151.2), "equator": (0.0, 0.0), "north pole": (90.0, 0.0),
          "south pole": (-90.0, 45.0), "antimeridian +": (10.0, 180.0), "antimeridian -": (-20.0, -180.0),
          "beside the antimeridian": (64.0, 179.9995)}


def cases():
    out = []

    def add(name, frame, fx, limit=LIMIT, time=12.5):
        out.append((name, limit, frame, fx, time))

    icao = 0x4B1A00
    # every type code and both CPR formats, honest (15 m away) and displaced (5 km away); downlink formats that are not 17
    for tc in range(32):
        for odd in (0, 1):
            for shift_m in (15.0, 5000.0):
                lat, lon = F.destination(PLACES["mid"], shift_m / 1852.0, 75.0 + tc)
                add(f"tc {tc} odd {odd} {shift_m:.0f} m", M.position_frame(icao + tc, tc, odd, lat, lon),
                    M.fix(*PLACES["mid"], flags=GOOD | (M.FIX_ALTITUDE if tc & 1 else 0)))
    for df in (0, 4, 11, 16, 18, 19, 20, 21, 24, 31):
        add(f"df {df}", M.position_frame(icao, 11, 0, *PLACES["mid"], df=df), M.fix(*PLACES["mid"]))
    # fixes at the poles, the equator and the antimeridian, with the report on every side of them
    for name, (plat, plon) in PLACES.items():
        for bearing in (0.0, 90.0, 180.0, 270.0, 33.0):
            for shift_m in (0.0, 30.0, 2500.0, 90000.0):
                lat, lon = F.destination((plat, plon), shift_m / 1852.0, bearing)
                for odd in (0, 1):
                    add(f"{name} {bearing:.0f} deg {shift_m:.0f} m odd {odd}",
                        M.position_frame(icao, 11 + odd, odd, lat, lon), M.fix(plat, plon, height_m=123.456789))
    # the fix exactly half a latitude zone from the report, on either side (6 degrees even, 360/59 odd), and just inside
    for odd, j, y in ((0, 7, 0.25), (0, -3, 0.5), (1, 5, 0.125)):
        d_lat = 360.0 / (60 - odd)
        rlat = d_lat * (j + y)
        for side in (-0.5, 0.5, -0.48, 0.48):
            add(f"half a zone odd {odd} j {j} side {side}", M.cpr_frame(icao, 13, odd, int(y * 131072), 0x8000),
                M.fix(rlat + side * d_lat, 10.0))
    # ... and half a longitude zone at the equator's neighbour latitude (NL = 59: zones of 360 / 59 and 360 / 58 degrees)
    for odd in (0, 1):
        d_lon = 360.0 / (59 - odd)
        for side in (-0.5, 0.5, -0.49, 0.49):
            add(f"half a longitude zone odd {odd} side {side}", M.cpr_frame(icao, 13, odd, 0x100, 0x4000),
                M.fix(0.01, d_lon * (3 + 0.125 + side)))
    # FAR: the decode lands beyond 180 NM, or above 90 degrees
    add("far: 3 degrees of latitude", M.cpr_frame(icao, 11, 0, int(0.25 * 131072), 0), M.fix(46.5, 0.0))
    add("far: above the pole", M.cpr_frame(icao, 11, 0, int(0.3 * 131072), 0), M.fix(89.9, 0.0))
    add("far: below the south pole", M.cpr_frame(icao, 11, 0, int(0.7 * 131072), 0), M.fix(-89.9, 0.0))
    # fields that are not numbers or off the globe; the fix is still the newest valid one and is kept as it is
    nan, inf = math.nan, math.inf
    for name, kw in (("nan latitude", dict(latitude=nan)), ("nan longitude", dict(longitude=nan)),
                     ("inf latitude", dict(latitude=inf)), ("-inf longitude", dict(longitude=-inf)),
                     ("latitude 90.5", dict(latitude=90.5)), ("longitude -180.5", dict(longitude=-180.5)),
                     ("nan height", dict(height_m=nan)), ("inf height", dict(height_m=inf)),
                     ("height beyond f32", dict(height_m=1e300)), ("nan residual", dict(residual_rms_m=nan)),
                     ("inf pdop", dict(pdop=inf))):
        base = dict(latitude=47.3, longitude=8.5)
        base.update(kw)
        add(name, M.position_frame(icao, 11, 0, 47.3, 8.5), M.fix(**base))
    # each outcome flag of the solver on its own, and the combinations it really gives
    lat, lon = F.destination(PLACES["mid"], 3000.0 / 1852.0, 10.0)
    for flags in [1 << b for b in range(10)] + [0, GOOD, GOOD | M.FIX_ALTITUDE, 0x1 | 0x20, 0x1 | 0x2 | 0x40,
                                                 0x1 | 0x2 | 0x80, 0x1 | 0x4 | 0x2 | 0x40, 0x200 | 0x8, 0x3FF]:
        add(f"fix flags {flags:#x}", M.position_frame(icao, 11, 1, lat, lon), M.fix(*PLACES["mid"], flags=flags, n_used=4))
    # the limit itself: the same 3 km under limits on either side of it
    for limit in (100.0, 2000.0, 6000.0, 1e9, 1e-3):
        add(f"limit {limit}", M.position_frame(icao, 11, 1, lat, lon), M.fix(*PLACES["mid"]), limit=limit)
    return out


LIAR, VELOCITY_ONLY, IDENT_ONLY = 0x400003, 0x400007, 0x400008


def network(oracle, spt=1e-9, displaced_deg=0.05, seed=21, **kw):
    """A clock-sync scenario of tests/clock_cases.py (8 receivers, every message heard by all) whose 160 messages belong
    to 16 aircraft: 13 honest ones, LIAR reports positions displaced_deg north of where it is, VELOCITY_ONLY sends
    airborne-velocity messages only and IDENT_ONLY identification messages only.  kw: further keywords of the scenario."""
    from tests import clock_cases as H
    from tests import mlat_cases
    from tests import mlat_model
    from tests import traffic

    def frames_of(oracle, pos):
        out = []
        for i, p in enumerate(pos):
            icao = 0x400000 + i % 16
            h, _, phi, lam = mlat_model.geodetic_of(p)
            lat, lon = math.degrees(phi) + (displaced_deg if icao == LIAR else 0.0), math.degrees(lam)
            if icao == VELOCITY_ONLY:
                out.append(F.raw_frame(oracle, icao, 19 << 51 | 1 << 48 | (100 + i) << 21 | (200 + i)))
            elif icao == IDENT_ONLY:
                out.append(F.raw_frame(oracle, icao, 4 << 51 | i))
            else:
                yz, xz = F.cpr_encode(lat, lon, (i // 16) & 1, False)
                out.append(traffic.position_frame(oracle, icao, (i // 16) & 1, yz, xz,
                                                  alt_code=mlat_cases.altitude_code(h)[0]))
        return out

    return H.scenario(oracle, 8, 160, seed=seed, p_heard=1.0, frames_of=frames_of, spt=spt, **kw)
