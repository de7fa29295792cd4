"""Multilaterated positions per aircraft (include/adsb_hip.h, "Multilaterated positions per aircraft"): a plain Python
restatement of the per-frame step (counted, valid, checked, disagreement, FAR) and of the merge as a sequential loop per
aircraft.  The local CPR decode the check is defined by is tests/fix_model.py's restatement of the header's formulas, with
the solved position as the site; nothing here reads the library."""
import math

import numpy as np

from tests import fix_model as F

VALID, ALTITUDE, CHECKED, DISAGREE, FAR = 0x1, 0x2, 0x4, 0x8, 0x10     # ADSB_TRACK_MLAT_*
FIX_ATTEMPTED, FIX_ALTITUDE, FIX_VALID = 0x1, 0x4, 0x100                 # ADSB_MLAT_* read by the merge
FAR_M = np.float32(333360.0)                                            # 180 NM
U32 = (1 << 32) - 1
# the 64-byte adsb_mlat_fix, the 64-byte adsb_aircraft_mlat and the 16-byte adsb_frame_mlat, written out here so the model
# does not depend on the library
FIX_DTYPE = np.dtype([("latitude", "<f8"), ("longitude", "<f8"), ("height_m", "<f8"), ("time_s", "<f8"),
                      ("residual_rms_m", "<f4"), ("pdop", "<f4"), ("hdop", "<f4"), ("vdop", "<f4"), ("n_used", "<u2"),
                      ("iterations", "<u2"), ("flags", "<u4"), ("reserved", "<u8")])
OFFSETS = {"time": 0, "latitude": 8, "longitude": 16, "height_m": 24, "residual_rms_m": 28, "pdop": 32,
           "last_disagreement_m": 36, "max_disagreement_m": 40, "n_attempted": 44, "n_valid": 48, "n_checked": 52,
           "n_disagree": 56, "n_used": 60, "flags": 62, "reserved": 63}
MODEL_DTYPE = np.dtype({"names": list(OFFSETS),
                        "formats": ["<f8", "<f8", "<f8", "<f4", "<f4", "<f4", "<f4", "<f4", "<u4", "<u4", "<u4", "<u4",
                                    "<u2", "u1", "u1"],
                        "offsets": list(OFFSETS.values()), "itemsize": 64})
FRAME_DTYPE = np.dtype([("disagreement_m", "<f4"), ("icao", "<u4"), ("flags", "<u4"), ("reserved", "<u4")])
EXACT = ("time", "latitude", "longitude", "height_m", "residual_rms_m", "pdop", "n_attempted", "n_valid", "n_checked",
         "n_disagree", "n_used", "flags", "reserved")                   # compared bit for bit (NaN-aware: as bytes)
assert MODEL_DTYPE.itemsize == 64 and FRAME_DTYPE.itemsize == 16 and FIX_DTYPE.itemsize == 64


def fix(latitude=0.0, longitude=0.0, height_m=10000.0, flags=FIX_ATTEMPTED | 0x2 | FIX_VALID, residual_rms_m=3.0,
        pdop=1.5, n_used=5):
    """One adsb_mlat_fix record (the solver's other outputs are not read by the merge; they get plain values)."""
    f = np.zeros((), dtype=FIX_DTYPE)
    f["latitude"], f["longitude"], f["height_m"], f["flags"] = latitude, longitude, height_m, flags
    f["residual_rms_m"], f["pdop"], f["n_used"] = residual_rms_m, pdop, n_used
    f["time_s"], f["hdop"], f["vdop"], f["iterations"] = -1e-4, 1.0, 1.1, 7
    return f


def site_ok(lat, lon):
    """(lat, lon, 180 NM) is a site a fixes reserve accepts (a NaN fails every comparison)."""
    return -90.0 <= lat <= 90.0 and -180.0 <= lon <= 180.0


def frame_check(limit_m, frame, fx):
    """One counted frame and its fix -> (adsb_frame_mlat.flags, disagreement_m as np.float32, 1 if the fix was
    attempted)."""
    attempted = 1 if int(fx["flags"]) & FIX_ATTEMPTED else 0
    if not int(fx["flags"]) & FIX_VALID:
        return 0, np.float32(0.0), attempted
    lat, lon = float(fx["latitude"]), float(fx["longitude"])
    if not site_ok(lat, lon):
        return VALID, np.float32(0.0), attempted
    d = F.decode((lat, lon, 180.0), bytes(frame))
    if d is None or d["flags"] & F.SURFACE:                              # no airborne position message
        return VALID, np.float32(0.0), attempted
    if d["flags"] & F.REJECTED:                                          # |lat| > 90, or beyond 180 NM
        return VALID | CHECKED | FAR | DISAGREE, FAR_M, attempted
    metres = d["range"] * 1852.0
    return VALID | CHECKED | (DISAGREE if metres > limit_m else 0), np.float32(metres), attempted


def empty():
    a = np.zeros((), dtype=MODEL_DTYPE)
    a["time"] = np.nan
    return a


def merge(a, limit_m, frame, fx, time):
    """The aircraft's record `a` after one more counted frame with fix fx, heard at `time`."""
    flags, dis, attempted = frame_check(limit_m, frame, fx)
    a = a.copy()
    a["n_attempted"] = min(int(a["n_attempted"]) + attempted, U32)
    if flags & VALID:
        a["n_valid"] = min(int(a["n_valid"]) + 1, U32)
        a["time"], a["latitude"], a["longitude"] = time, fx["latitude"], fx["longitude"]
        with np.errstate(over="ignore", invalid="ignore"):
            a["height_m"] = np.float32(fx["height_m"])
        a["residual_rms_m"], a["pdop"], a["n_used"] = fx["residual_rms_m"], fx["pdop"], fx["n_used"]
        a["flags"] = (int(a["flags"]) & CHECKED) | VALID | (ALTITUDE if int(fx["flags"]) & FIX_ALTITUDE else 0)
    if flags & CHECKED:
        a["n_checked"] = min(int(a["n_checked"]) + 1, U32)
        if flags & DISAGREE:
            a["n_disagree"] = min(int(a["n_disagree"]) + 1, U32)
        a["last_disagreement_m"] = dis
        a["max_disagreement_m"] = max(np.float32(a["max_disagreement_m"]), dis)
        a["flags"] = int(a["flags"]) | CHECKED
    return a


def record_of(limit_m, frame, fx, time):
    """What adsb_host_track_mlat_of returns: (the record of an aircraft whose only counted frame is this one, the frame's
    flags, its disagreement_m)."""
    flags, dis, _ = frame_check(limit_m, frame, fx)
    return merge(empty(), limit_m, frame, fx, time), flags, dis


def apply(state, limit_m, frames, fixes, sample_base=0, sps=0.5e-6, untracked=None, step=merge):
    """One update_mlat over `frames` (fields offset and bytes) and `fixes` into state {icao: MODEL_DTYPE scalar}, in
    list order; every tracked frame admits its aircraft.  step: merge, or a function of the same arguments (the GPU tests
    pass one built on the CPU mirror).  Returns the state."""
    icaos = F.frame_icaos(frames)
    for k in range(len(frames)):
        if untracked is not None and untracked[k]:
            continue
        icao = int(icaos[k])
        time = float(int(sample_base) + int(frames["offset"][k])) * sps
        state[icao] = step(state.get(icao, empty()), limit_m, frames["bytes"][k].tobytes(), fixes[k], time)
    return state


def records(state, icaos):
    out = np.zeros(len(icaos), dtype=MODEL_DTYPE)
    for k, icao in enumerate(icaos):
        out[k] = state.get(int(icao), empty())
    return out


def frame_records(limit_m, frames, fixes, untracked=None, check=frame_check):
    """What frame_mlat() returns for the frames of one update_mlat."""
    out = np.zeros(len(frames), dtype=FRAME_DTYPE)
    out["icao"] = F.frame_icaos(frames)
    for k in range(len(frames)):
        if untracked is not None and untracked[k]:
            continue
        out[k]["flags"], out[k]["disagreement_m"] = check(limit_m, frames["bytes"][k].tobytes(), fixes[k])[:2]
    return out


def f32_step(x):
    """The distance from |x| to the next f32 above it."""
    return float(np.spacing(np.abs(np.float32(x))))


def assert_records_equal(got, want, tol_of, what=""):
    """Every field but the two disagreements bit for bit (NaN-aware); those within tol_of(the expected value)."""
    assert len(got) == len(want) and got.dtype.itemsize == want.dtype.itemsize == 64, (what, len(got), len(want))
    for name in EXACT:
        g, w = np.ascontiguousarray(got[name]), np.ascontiguousarray(want[name])
        assert g.tobytes() == w.tobytes(), (what, name, np.nonzero(g.view(f"u{g.itemsize}") != w.view(f"u{w.itemsize}"))[0][:5])
    for name in ("last_disagreement_m", "max_disagreement_m"):
        for k in range(len(got)):
            assert abs(float(got[name][k]) - float(want[name][k])) <= tol_of(want[name][k]), \
                (what, name, k, got[name][k], want[name][k])


def assert_frames_equal(got, want, tol_of, what=""):
    assert len(got) == len(want) and got.dtype.itemsize == 16, (what, len(got), len(want))
    for name in ("icao", "flags", "reserved"):
        assert np.array_equal(got[name], want[name]), (what, name, np.nonzero(got[name] != want[name])[0][:5])
    for k in range(len(got)):
        assert abs(float(got["disagreement_m"][k]) - float(want["disagreement_m"][k])) <= tol_of(want["disagreement_m"][k]), \
            (what, k, got["disagreement_m"][k], want["disagreement_m"][k])


# ---- traffic (the CRC is not read by the tracker: frames here carry none) ------------------------------------------------
def raw_frame(icao, me, df=17):
    return bytes([df << 3 | 5, (icao >> 16) & 0xFF, (icao >> 8) & 0xFF, icao & 0xFF]) + int(me).to_bytes(7, "big") + bytes(3)


def position_frame(icao, tc, odd, lat, lon, df=17, alt_code=0x3A8):
    """A position-shaped message (ME: TC, altitude code, F, lat_cpr, lon_cpr by the AIRBORNE encoder) of an aircraft at
    (lat, lon), whatever tc and df say it is."""
    yz, xz = F.cpr_encode(lat, lon, odd, False)
    return raw_frame(icao, tc << 51 | alt_code << 36 | odd << 34 | yz << 17 | xz, df)


def cpr_frame(icao, tc, odd, lat_cpr, lon_cpr, df=17):
    return raw_frame(icao, tc << 51 | 0x3A8 << 36 | odd << 34 | lat_cpr << 17 | lon_cpr, df)


def frames_array(items, dtype):
    """[(offset, 14 frame bytes)] -> an array of `dtype` (fields offset, bytes; fixed_bit if it has one)."""
    out = np.zeros(len(items), dtype=dtype)
    for k, (off, b) in enumerate(items):
        out[k]["offset"] = off
        out[k]["bytes"] = np.frombuffer(bytes(b), dtype=np.uint8)
    if "fixed_bit" in (dtype.names or ()):
        out["fixed_bit"] = 0xFF
    return out


def traffic(seed, n_frames, icaos, limit_m=1000.0, step=40):
    """A time-ordered list of n_frames frames of the given aircraft around (47, 8) with a fix for each: honest airborne
    position messages (below 50 m from the fix), displaced ones (2.5 km and more), velocity and identification messages,
    and fixes that are valid, attempted but not valid, or not attempted.  -> ([(offset, bytes)], FIX_DTYPE array)"""
    rng = np.random.default_rng(seed)
    icaos = [int(x) for x in icaos]
    pos = {a: (47.0 + float(rng.uniform(-1, 1)), 8.0 + float(rng.uniform(-1.5, 1.5))) for a in icaos}
    items, fixes = [], np.zeros(n_frames, dtype=FIX_DTYPE)
    for k in range(n_frames):
        a = icaos[int(rng.integers(0, len(icaos)))]
        lat, lon = pos[a]
        what = rng.random()
        if what < 0.55:
            shift = float(rng.uniform(2.5, 40.0)) / 1.852 if rng.random() < 0.25 else 0.0   # NM
            rlat, rlon = F.destination((lat, lon), shift, float(rng.uniform(0, 360))) if shift else (lat, lon)
            fr = position_frame(a, int(rng.choice([9, 11, 18, 20, 22])), int(rng.integers(0, 2)), rlat, rlon)
        elif what < 0.75:
            fr = raw_frame(a, 19 << 51 | int(rng.integers(1, 5)) << 48 | int(rng.integers(0, 1 << 48)))
        elif what < 0.9:
            fr = raw_frame(a, 4 << 51 | int(rng.integers(0, 1 << 48)))
        else:
            fr = position_frame(a, int(rng.integers(5, 9)), int(rng.integers(0, 2)), lat, lon)   # surface: not checked
        items.append((100 + step * (k - (1 if k % 3 == 2 else 0)), fr))   # every third frame shares its offset
        kind = rng.random()
        if kind < 0.6:     # the solver's position: within 20 m of the truth
            flat, flon = F.destination((lat, lon), float(rng.uniform(0, 20.0)) / 1852.0, float(rng.uniform(0, 360)))
            fixes[k] = fix(flat, flon, float(rng.uniform(0, 12000)), FIX_ATTEMPTED | 0x2 | FIX_VALID |
                           (FIX_ALTITUDE if rng.random() < 0.5 else 0), float(rng.uniform(0, 50)), float(rng.uniform(1, 9)),
                           int(rng.integers(3, 9)))
        elif kind < 0.8:   # attempted, not valid
            fixes[k] = fix(lat + 1.0, lon, 0.0, FIX_ATTEMPTED | int(rng.choice([0x20, 0x2 | 0x40, 0x2 | 0x80])))
        else:              # not attempted
            fixes[k] = fix(0.0, 0.0, 0.0, int(rng.choice([0x8, 0x10, 0x200])), 0.0, 0.0, int(rng.integers(0, 3)))
    return items, fixes
