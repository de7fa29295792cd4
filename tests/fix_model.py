"""Positions from single messages (include/adsb_hip.h, "Positions from single messages"): a plain Python restatement of
the locally unambiguous CPR decode with range and bearing from the site, the per-aircraft merge, and what the tests need
to make traffic for it: a CPR ENCODER written from DO-260's definition (not the inverse of the decode under test), a
frame builder for surface and airborne position messages with a correct CRC, and points at a given range and bearing."""
import math

import numpy as np

VALID, SURFACE, ALT, SPEED, TRACK, REJECTED = 1, 2, 4, 8, 16, 32
R_NM = 3440.065
# the 64-byte adsb_fix and the 32-byte adsb_frame_fix, written out here so the model does not depend on the library
OFFSETS = {"time": 0, "latitude": 8, "longitude": 16, "range_nm": 24, "bearing_deg": 28, "ground_speed_kt": 32,
           "track_deg": 36, "altitude": 40, "n_fixes": 44, "n_rejected": 48, "type_code": 52, "flags": 53, "cpr_odd": 54,
           "reserved8": 55, "reserved": 56}
# (_pad: the C struct's four bytes of tail padding, a field here so that every copy carries them)
MODEL_DTYPE = np.dtype({"names": list(OFFSETS) + ["_pad"],
                        "formats": ["<f8", "<f8", "<f8", "<f4", "<f4", "<f4", "<f4", "<i4", "<u4", "<u4", "u1", "u1",
                                    "u1", "u1", "<u4", "<u4"],
                        "offsets": list(OFFSETS.values()) + [60], "itemsize": 64})
FRAME_DTYPE = np.dtype([("latitude", "<f8"), ("longitude", "<f8"), ("range_nm", "<f4"), ("bearing_deg", "<f4"),
                        ("icao", "<u4"), ("flags", "<u4")])
EXACT = ("ground_speed_kt", "track_deg", "altitude", "n_fixes", "n_rejected", "type_code", "flags", "cpr_odd",
         "reserved8", "reserved", "_pad")                          # compared bit for bit; time too (NaN-aware)
U32 = (1 << 32) - 1
# the seven sites of the host test: one within 0.1 degree of the antimeridian, one within 0.05 degree of the equator and
# the prime meridian, one above 75 N
SITES = [(-43.5, 172.5, 180.0), (0.01, -0.02, 180.0), (51.5, -0.1, 120.0), (64.1, -21.9, 180.0), (-33.9, 151.2, 60.0),
         (1.3, 179.95, 180.0), (78.2, 15.6, 150.0)]


def num_zones(lat):
    """NL (cpr.rs:39-54)"""
    if lat == 0.0:
        return 59
    if abs(lat) == 87.0:
        return 2
    if abs(lat) > 87.0:
        return 1
    a = 1.0 - math.cos(math.pi / 30.0)
    b = math.cos(math.pi / 180.0 * lat)
    return int(math.floor((2.0 * math.pi) / math.acos(1.0 - (a / (b * b)))))


def mod(a, b):
    return a - b * math.floor(a / b)


def movement_kt(m):
    """Surface movement field -> knots, None for 'no speed'."""
    if m == 0 or m >= 125:
        return None
    if m == 1:
        return 0.0
    if m <= 8:
        return 0.125 + (m - 2) * 0.125
    if m <= 12:
        return 1.0 + (m - 9) * 0.25
    if m <= 38:
        return 2.0 + (m - 13) * 0.5
    if m <= 93:
        return 15.0 + (m - 39)
    if m <= 108:
        return 70.0 + (m - 94) * 2.0
    if m <= 123:
        return 100.0 + (m - 109) * 5.0
    return 175.0


def range_bearing(lat1, lon1, lat2, lon2):
    """(haversine distance in NM, initial bearing in degrees in [0, 360)) in f64"""
    p1, p2, dl = math.radians(lat1), math.radians(lat2), math.radians(lon2 - lon1)
    h = math.sin((p2 - p1) / 2.0) ** 2 + math.cos(p1) * math.cos(p2) * math.sin(dl / 2.0) ** 2
    rng = 2.0 * R_NM * math.asin(min(1.0, math.sqrt(h)))
    brg = math.degrees(math.atan2(math.sin(dl) * math.cos(p2),
                                  math.cos(p1) * math.sin(p2) - math.sin(p1) * math.cos(p2) * math.cos(dl)))
    if brg < 0.0:
        brg += 360.0
    if brg >= 360.0:
        brg -= 360.0
    return rng, brg


def bearing_f32(brg):
    """The f64 bearing rounded to f32 once; a rounding that gives 360 is 0, so the result stays in [0, 360)."""
    b = np.float32(brg)
    return np.float32(0.0) if b >= np.float32(360.0) else b


def bits(frame):
    """ME bit fields of a frame (bit 0 = the top bit of frame byte 4)."""
    me = int.from_bytes(bytes(frame)[4:11], "big")
    return lambda first, width: (me >> (56 - first - width)) & ((1 << width) - 1)


def local_position(site, odd, surface, lat_cpr, lon_cpr):
    """(lat, lon, dLat, dLon) of the header's formulas; lon is None if |lat| > 90."""
    span = 90.0 if surface else 360.0
    y, x = lat_cpr / 131072.0, lon_cpr / 131072.0
    d_lat = span / (60 - odd)
    j = math.floor(site[0] / d_lat) + math.floor(0.5 + mod(site[0], d_lat) / d_lat - y)
    lat = d_lat * (j + y)
    if not abs(lat) <= 90.0:
        return lat, None, d_lat, None
    d_lon = span / max(num_zones(lat) - odd, 1)
    m = math.floor(site[1] / d_lon) + math.floor(0.5 + mod(site[1], d_lon) / d_lon - x)
    lon = d_lon * (m + x)
    while lon < -180.0:
        lon += 360.0
    while lon > 180.0:
        lon -= 360.0
    return lat, lon, d_lat, d_lon


def decode(site, frame):
    """One frame against one site (latitude, longitude, max_range_nm): None for a frame that is no position message,
    else a dict with "flags" (REJECTED | SURFACE for a rejected one, and then nothing else) and, accepted, latitude,
    longitude, range (f64), bearing (f64), ground_speed_kt, track_deg, altitude, type_code, cpr_odd."""
    frame = bytes(frame)
    f = bits(frame)
    tc = f(0, 5)
    surface = 5 <= tc <= 8
    if frame[0] >> 3 != 17 or not (surface or 9 <= tc <= 18 or 20 <= tc <= 22):
        return None
    odd = f(21, 1)
    kind = SURFACE if surface else 0
    lat, lon, _, _ = local_position(site, odd, surface, f(22, 17), f(39, 17))
    if lon is None:
        return {"flags": REJECTED | kind, "range": math.inf}
    rng, brg = range_bearing(site[0], site[1], lat, lon)
    if rng > (min(site[2], 45.0) if surface else site[2]):
        return {"flags": REJECTED | kind, "range": rng}
    out = {"flags": VALID | kind, "latitude": lat, "longitude": lon, "range": rng, "bearing": brg, "ground_speed_kt": 0.0,
           "track_deg": 0.0, "altitude": 0, "type_code": tc, "cpr_odd": odd}
    if surface:
        kt = movement_kt(f(5, 7))
        if kt is not None:
            out["ground_speed_kt"] = kt
            out["flags"] |= SPEED
        if f(12, 1):
            out["track_deg"] = f(13, 7) * 360.0 / 128.0
            out["flags"] |= TRACK
    elif tc <= 18:
        out["altitude"] = (f(8, 7) << 4 | f(16, 4)) * (25 if f(15, 1) else 100) - 1000
        out["flags"] |= ALT
    return out


def empty():
    a = np.zeros((), dtype=MODEL_DTYPE)
    a["time"] = np.nan
    return a


def merge(a, d, time):
    """The aircraft's fix `a` (a MODEL_DTYPE scalar) after one more frame whose decode is d, heard at `time`."""
    if d is None:
        return a
    a = a.copy()
    if d["flags"] & REJECTED:
        a["n_rejected"] = min(int(a["n_rejected"]) + 1, U32)
        return a
    a["time"], a["latitude"], a["longitude"] = time, d["latitude"], d["longitude"]
    a["range_nm"], a["bearing_deg"] = np.float32(d["range"]), bearing_f32(d["bearing"])
    a["ground_speed_kt"], a["track_deg"] = np.float32(d["ground_speed_kt"]), np.float32(d["track_deg"])
    a["altitude"], a["type_code"], a["flags"], a["cpr_odd"] = d["altitude"], d["type_code"], d["flags"], d["cpr_odd"]
    a["n_fixes"] = min(int(a["n_fixes"]) + 1, U32)
    return a


def fix_of(site, frame, time):
    """What adsb_host_fix_of returns: (the fix of an aircraft whose only frame is this one, the frame's flags)."""
    d = decode(site, frame)
    return merge(empty(), d, time), (0 if d is None else d["flags"])


def frame_icaos(frames):
    b = frames["bytes"].astype(np.uint32)
    return b[:, 1] << 16 | b[:, 2] << 8 | b[:, 3]


def apply(state, site, frames, sample_base=0, sps=0.5e-6, untracked=None):
    """One update of a table with `site` over `frames` (fields offset and bytes) into state {icao: MODEL_DTYPE scalar}, in
    list order; every tracked frame admits its aircraft.  Returns the state."""
    icaos = frame_icaos(frames)
    for k in range(len(frames)):
        if untracked is not None and untracked[k]:
            continue
        icao = int(icaos[k])
        time = float(int(sample_base) + int(frames["offset"][k])) * sps
        state[icao] = merge(state.get(icao, empty()), decode(site, frames["bytes"][k].tobytes()), time)
    return state


def records(state, icaos):
    out = np.zeros(len(icaos), dtype=MODEL_DTYPE)
    for k, icao in enumerate(icaos):
        out[k] = state.get(int(icao), empty())
    return out


def frame_records(site, frames, untracked=None):
    """What frame_fixes() returns for one receiver's frames."""
    out = np.zeros(len(frames), dtype=FRAME_DTYPE)
    out["icao"] = frame_icaos(frames)
    for k in range(len(frames)):
        d = None if untracked is not None and untracked[k] else decode(site, frames["bytes"][k].tobytes())
        if d is None:
            continue
        out[k]["flags"] = d["flags"]
        if d["flags"] & VALID:
            out[k]["latitude"], out[k]["longitude"] = d["latitude"], d["longitude"]
            out[k]["range_nm"], out[k]["bearing_deg"] = np.float32(d["range"]), bearing_f32(d["bearing"])
    return out


def assert_fixes_equal(got, want, what=""):
    """Integers, flags, f32 surface fields and the time bit for bit; latitude and longitude equal as doubles (nothing in
    the decode before NL uses a math library and NL is an integer: device, mirror and model gave the same bits on every
    case of tests/fix_cases.py); range within 1e-4 NM; bearing within 1e-4 degree where the range is at least 1 NM (and
    modulo 360)."""
    assert len(got) == len(want) and got.dtype.itemsize == want.dtype.itemsize == 64, (what, len(got), len(want))
    for name in EXACT:
        assert np.array_equal(got[name], want[name]), (what, name, np.nonzero(got[name] != want[name])[0][:5])
    assert got["time"].tobytes() == want["time"].tobytes(), what
    assert not got["_pad"].any() and not got["reserved"].any() and not got["reserved8"].any(), what
    _assert_positions(got, want, what)


def _assert_positions(got, want, what):
    assert np.array_equal(got["latitude"], want["latitude"]), what
    assert np.array_equal(got["longitude"], want["longitude"]), what
    assert np.all(np.abs(got["range_nm"].astype(np.float64) - want["range_nm"]) <= 1e-4), what
    far = want["range_nm"] >= 1.0
    diff = np.abs(got["bearing_deg"].astype(np.float64) - want["bearing_deg"])[far]
    assert np.all(np.minimum(diff, 360.0 - diff) <= 1e-4), what


def assert_frame_fixes_equal(got, want, what=""):
    assert len(got) == len(want) and got.dtype.itemsize == 32, (what, len(got), len(want))
    assert np.array_equal(got["icao"], want["icao"]) and np.array_equal(got["flags"], want["flags"]), what
    _assert_positions(got, want, what)


# ---- traffic ------------------------------------------------------------------------------------------------------------
def cpr_encode(lat, lon, odd, surface):
    """DO-260's encoder: YZ = floor(2^Nb mod(lat, dLat) / dLat + 0.5), XZ likewise with NL of the re-quantised latitude;
    Nb = 17 airborne, 19 with the low 17 bits kept for surface.  -> (lat_cpr, lon_cpr)"""
    nb = 19 if surface else 17
    d_lat = 360.0 / (60 - odd)
    yz = math.floor(2 ** nb * mod(lat, d_lat) / d_lat + 0.5)
    rlat = d_lat * (yz / 2 ** nb + math.floor(lat / d_lat))
    d_lon = 360.0 / max(num_zones(rlat) - odd, 1)
    xz = math.floor(2 ** nb * mod(lon, d_lon) / d_lon + 0.5)
    return int(yz) & 0x1FFFF, int(xz) & 0x1FFFF


def destination(site, range_nm, bearing_deg):
    """The point `range_nm` from the site on the initial bearing `bearing_deg` (great circle), longitude in [-180, 180)."""
    d, b = range_nm / R_NM, math.radians(bearing_deg)
    p1, l1 = math.radians(site[0]), math.radians(site[1])
    p2 = math.asin(math.sin(p1) * math.cos(d) + math.cos(p1) * math.sin(d) * math.cos(b))
    l2 = l1 + math.atan2(math.sin(b) * math.sin(d) * math.cos(p1), math.cos(d) - math.sin(p1) * math.sin(p2))
    return math.degrees(p2), (math.degrees(l2) + 180.0) % 360.0 - 180.0


def with_crc(oracle, data11):
    crc = oracle.get_adsb_crc(data11)
    return data11 + bytes([(crc >> 16) & 0xFF, (crc >> 8) & 0xFF, crc & 0xFF])


def raw_frame(oracle, icao, me, df=17):
    """A frame with downlink format df, CA 5 and the 56-bit ME field `me`, with a correct CRC."""
    return with_crc(oracle, bytes([df << 3 | 5, (icao >> 16) & 0xFF, (icao >> 8) & 0xFF, icao & 0xFF]) +
                    int(me).to_bytes(7, "big"))


def position_frame(oracle, icao, tc, odd, lat_cpr, lon_cpr, alt_code=0x3A8, movement=0, track_valid=0, track=0):
    """A DF17 position message: surface for TC 5-8 (movement, track status, track), else airborne (12-bit altitude
    code)."""
    me = tc << 51 | odd << 34 | lat_cpr << 17 | lon_cpr
    if 5 <= tc <= 8:
        me |= movement << 44 | track_valid << 43 | track << 36
    else:
        me |= alt_code << 36
    return raw_frame(oracle, icao, me)


def frame_at(oracle, icao, site, range_nm, bearing_deg, tc, odd, **kw):
    """A position message of an aircraft `range_nm` from the site on `bearing_deg`."""
    lat, lon = destination(site, range_nm, bearing_deg)
    yz, xz = cpr_encode(lat, lon, odd, 5 <= tc <= 8)
    return position_frame(oracle, icao, tc, odd, yz, xz, **kw)


def random_frame(oracle, rng, icao):
    """Any type code 0-31 with the other 51 ME bits random: both CPR formats, every raw movement, track valid or not,
    positions anywhere in the zone around the site; one in a hundred is not DF 17."""
    me = int(rng.integers(0, 32)) << 51 | int(rng.integers(0, 1 << 51))
    return raw_frame(oracle, icao, me, df=17 if rng.random() >= 0.01 else int(rng.choice([11, 18, 20])))


def mixed_traffic(oracle, seed, site, n_aircraft, n_frames, span_s=60.0, sps=0.5e-6):
    """A time-ordered FRAME list (offset, bytes, fixed_bit = 0xFF; status 0) of n_aircraft aircraft near `site`: surface
    and airborne position messages (of aircraft mostly inside and sometimes outside the limits), velocity and
    identification messages and other type codes."""
    rng = np.random.default_rng(seed)
    icaos = [int(x) for x in rng.choice(np.arange(0x400000, 0x800000), size=n_aircraft, replace=False)]
    on_ground = rng.random(n_aircraft) < 0.3
    dist = np.where(on_ground, rng.uniform(0, 52, n_aircraft), rng.uniform(0, 1.15 * site[2], n_aircraft))
    brg = rng.uniform(0, 360, n_aircraft)
    out = np.zeros(n_frames, dtype=[("offset", "<u8"), ("bytes", "u1", (14,)), ("status", "u1"), ("fixed_bit", "u1")])
    out["fixed_bit"] = 0xFF
    out["offset"] = np.sort(rng.integers(0, int(span_s / sps), size=n_frames))
    for k in range(n_frames):
        a = int(rng.integers(0, n_aircraft))
        what = rng.random()
        if what < 0.65:
            tc = int(rng.integers(5, 9)) if on_ground[a] else int(rng.choice([9, 11, 13, 18, 20, 22]))
            fr = frame_at(oracle, icaos[a], site, float(dist[a]), float(brg[a]), tc, int(rng.integers(0, 2)),
                          alt_code=int(rng.integers(0, 1 << 12)), movement=int(rng.integers(0, 128)),
                          track_valid=int(rng.integers(0, 2)), track=int(rng.integers(0, 128)))
            dist[a] = abs(dist[a] + rng.normal(0, 0.05))
        elif what < 0.8:
            fr = raw_frame(oracle, icaos[a], 19 << 51 | int(rng.integers(1, 5)) << 48 | int(rng.integers(0, 1 << 48)))
        elif what < 0.9:
            fr = raw_frame(oracle, icaos[a], int(rng.integers(1, 5)) << 51 | int(rng.integers(0, 1 << 48)))
        else:
            fr = random_frame(oracle, rng, icaos[a])
        out[k]["bytes"] = np.frombuffer(fr, dtype=np.uint8)
    return out
