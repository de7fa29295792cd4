"""An independent model of the filter behind a table's multilaterated fixes (include/adsb_hip.h, "Filtered mlat track per
aircraft"), written from the header's formulas in Python floats and `math`; it shares no text with csrc/adsb_track_filter.h.
The records are written out here so the model does not depend on the library.  No device, no library."""
import math

import numpy as np

RUNNING, VELOCITY, HEIGHT = 0x1, 0x2, 0x4
USABLE, APPLIED, INIT, RESET, OUTLIER, SKIPPED = 0x100, 0x200, 0x400, 0x800, 0x1000, 0x2000
FIX_ATTEMPTED, FIX_CONVERGED, FIX_ALTITUDE, FIX_VALID = 0x1, 0x2, 0x4, 0x100
U32 = (1 << 32) - 1
WGS84_A = 6378137.0
WGS84_F = 1.0 / 298.257223563
WGS84_E2 = WGS84_F * (2.0 - WGS84_F)

DEFAULTS = dict(accel_h=3.0, accel_v=1.5, range_sigma_m=30.0, altitude_sigma_m=15.0, gate=4.0, reset_gap_s=30.0,
                init_speed_sigma_h=300.0, init_speed_sigma_v=30.0, max_hdop=20.0, max_vdop=50.0, max_outliers=3,
                min_run=4)

FIX_DTYPE = np.dtype([("latitude", "<f8"), ("longitude", "<f8"), ("height_m", "<f8"), ("time_s", "<f8"),
                      ("residual_rms_m", "<f4"), ("pdop", "<f4"), ("hdop", "<f4"), ("vdop", "<f4"), ("n_used", "<u2"),
                      ("iterations", "<u2"), ("flags", "<u4"), ("reserved", "<u8")])
RECORD_DTYPE = np.dtype([("time", "<f8"), ("latitude", "<f8"), ("longitude", "<f8"), ("height_m", "<f8"),
                         ("v_north", "<f8"), ("v_east", "<f8"), ("v_up", "<f8"), ("p_north", "<f8", (3,)),
                         ("p_east", "<f8", (3,)), ("p_up", "<f8", (3,)), ("n_applied", "<u4"), ("n_outlier", "<u4"),
                         ("n_reset", "<u4"), ("n_skipped", "<u4"), ("run", "<u4"), ("outliers_run", "<u4"),
                         ("last_nis", "<f4"), ("flags", "<u4"), ("reserved", "<u4", (8,))])
FRAME_DTYPE = np.dtype([("latitude", "<f8"), ("longitude", "<f8"), ("height_m", "<f4"), ("nis", "<f4"), ("flags", "<u4"),
                        ("reserved", "<u4")])
OPERAND_DTYPE = np.dtype([("time", "<f8"), ("latitude", "<f8"), ("longitude", "<f8"), ("rn", "<f8"), ("re", "<f8"),
                          ("var_h", "<f8"), ("var_v", "<f8"), ("height_m", "<f4"), ("flags", "<u4")])
assert RECORD_DTYPE.itemsize == 192 and FRAME_DTYPE.itemsize == 32 and OPERAND_DTYPE.itemsize == 64
# what is compared exactly, within the f64 bound, and within one f32 step
RECORD_EXACT = ("n_applied", "n_outlier", "n_reset", "n_skipped", "run", "outliers_run", "flags", "reserved")
RECORD_F64 = ("time", "latitude", "longitude", "height_m", "v_north", "v_east", "v_up", "p_north", "p_east", "p_up")
RECORD_F32 = ("last_nis",)
FRAME_EXACT, FRAME_F64, FRAME_F32 = ("flags", "reserved"), ("latitude", "longitude"), ("height_m", "nis")
OPERAND_EXACT = ("time", "latitude", "longitude", "height_m", "flags")
OPERAND_F64 = ("rn", "re", "var_h", "var_v")


def config(**kw):
    """The header's defaults with every given non-zero field in place."""
    c = dict(DEFAULTS)
    for k, v in kw.items():
        if k not in c:
            raise KeyError(k)
        if v:
            c[k] = v
    return c


def fix(latitude, longitude, height_m=10000.0, flags=FIX_ATTEMPTED | FIX_CONVERGED | FIX_VALID, residual_rms_m=3.0,
        hdop=1.0, vdop=2.0, pdop=2.5, n_used=5):
    f = np.zeros((), dtype=FIX_DTYPE)
    f["latitude"], f["longitude"], f["height_m"], f["flags"] = latitude, longitude, height_m, flags
    f["residual_rms_m"], f["hdop"], f["vdop"], f["pdop"], f["n_used"], f["iterations"] = residual_rms_m, hdop, vdop, pdop, n_used, 4
    return f


def empty():
    a = np.zeros((), dtype=RECORD_DTYPE)
    a["time"] = np.nan
    return a


def operand(c, fx, time, counted=True):
    """The header's PER FRAME: an OPERAND_DTYPE scalar, all zero for a frame that is not usable."""
    o = np.zeros((), dtype=OPERAND_DTYPE)
    flags = int(fx["flags"])
    lat, lon, h = float(fx["latitude"]), float(fx["longitude"]), float(fx["height_m"])
    hdop, vdop, res = float(fx["hdop"]), float(fx["vdop"]), float(fx["residual_rms_m"])
    if not counted or not flags & FIX_VALID:
        return o
    if not (math.isfinite(lat) and math.isfinite(lon) and math.isfinite(h)) or abs(lat) > 89.0:
        return o
    if h < -1000.0 or h > 100000.0 or not math.isfinite(hdop) or hdop <= 0.0 or hdop > c["max_hdop"]:
        return o
    sr = res if res > c["range_sigma_m"] else c["range_sigma_m"]            # a NaN residual compares false
    var_h = (hdop * sr) ** 2
    if not math.isfinite(var_h):
        return o
    altitude = bool(flags & FIX_ALTITUDE)
    var_v = c["altitude_sigma_m"] ** 2 if altitude else (vdop * sr) ** 2
    height = math.isfinite(var_v) and (altitude or 0.0 < vdop <= c["max_vdop"])
    if not height:
        var_v = (c["max_vdop"] * sr) ** 2
    s = math.sin(math.radians(lat))
    w2 = 1.0 - WGS84_E2 * s * s
    meridional = WGS84_A * (1.0 - WGS84_E2) / w2 ** 1.5
    prime_vertical = WGS84_A / math.sqrt(w2)
    o["time"], o["latitude"], o["longitude"], o["height_m"] = time, lat, lon, np.float32(h)
    o["rn"] = math.radians(meridional + h)
    o["re"] = math.radians((prime_vertical + h) * math.cos(math.radians(lat)))
    o["var_h"], o["var_v"] = var_h, var_v
    o["flags"] = USABLE | (HEIGHT if height else 0)
    return o


def _wrap(deg):
    return deg - 360.0 if deg > 180.0 else deg + 360.0 if deg < -180.0 else deg


def _inc(x):
    return min(int(x) + 1, U32)


def _predict(v, p, q, dt):
    ppp, ppv, pvv = (float(x) for x in p)
    return (v * dt, ppp + 2.0 * dt * ppv + dt ** 2 * pvv + q * dt ** 4 / 4.0, ppv + dt * pvv + q * dt ** 3 / 2.0,
            pvv + q * dt ** 2)


def _update(pred, y, s, v):
    """-> (displacement, velocity, (Ppp, Ppv, Pvv)) of a measured axis."""
    p, ppp, ppv, pvv = pred
    kp, kv = ppp / s, ppv / s
    return p + kp * y, v + kv * y, ((1.0 - kp) * ppp, (1.0 - kp) * ppv, pvv - kv * ppv)


def _start(c, a, o):
    a["time"], a["latitude"], a["longitude"], a["height_m"] = o["time"], o["latitude"], o["longitude"], float(o["height_m"])
    a["v_north"] = a["v_east"] = a["v_up"] = 0.0
    a["p_north"] = a["p_east"] = (float(o["var_h"]), 0.0, c["init_speed_sigma_h"] ** 2)
    a["p_up"] = (float(o["var_v"]), 0.0, c["init_speed_sigma_v"] ** 2)
    a["run"], a["outliers_run"] = 1, 0
    a["flags"] = RUNNING | (int(o["flags"]) & HEIGHT)


def step(c, a, o):
    """The header's PER AIRCRAFT for one frame: (the record after it, the frame's FRAME_DTYPE scalar)."""
    a = a.copy()
    f = np.zeros((), dtype=FRAME_DTYPE)
    if not int(o["flags"]) & USABLE:
        return a, f
    flags, nis, start = USABLE, 0.0, not int(a["flags"]) & RUNNING
    if not start:
        dt = float(o["time"]) - float(a["time"])
        if not dt >= 0.0:
            flags |= SKIPPED
            a["n_skipped"] = _inc(a["n_skipped"])
        elif dt > c["reset_gap_s"]:
            flags |= RESET
            a["n_reset"] = _inc(a["n_reset"])
            start = True
        else:
            qh, qv = c["accel_h"] ** 2, c["accel_v"] ** 2
            north = _predict(float(a["v_north"]), a["p_north"], qh, dt)
            east = _predict(float(a["v_east"]), a["p_east"], qh, dt)
            rn, re, var_h = float(o["rn"]), float(o["re"]), float(o["var_h"])
            yn = (float(o["latitude"]) - float(a["latitude"])) * rn - north[0]
            ye = _wrap(float(o["longitude"]) - float(a["longitude"])) * re - east[0]
            sn, se = north[1] + var_h, east[1] + var_h
            nis = yn * yn / sn + ye * ye / se
            a["last_nis"] = np.float32(nis)
            if nis > c["gate"] ** 2:
                flags |= OUTLIER
                a["n_outlier"], a["outliers_run"] = _inc(a["n_outlier"]), _inc(a["outliers_run"])
                if int(a["outliers_run"]) >= c["max_outliers"]:
                    flags |= RESET
                    a["n_reset"] = _inc(a["n_reset"])
                    start = True
            else:
                flags |= APPLIED
                up = _predict(float(a["v_up"]), a["p_up"], qv, dt)
                dn, a["v_north"], a["p_north"] = _update(north, yn, sn, float(a["v_north"]))
                de, a["v_east"], a["p_east"] = _update(east, ye, se, float(a["v_east"]))
                if int(o["flags"]) & HEIGHT:
                    yu = (float(o["height_m"]) - float(a["height_m"])) - up[0]
                    du, a["v_up"], a["p_up"] = _update(up, yu, up[1] + float(o["var_v"]), float(a["v_up"]))
                    a["flags"] = int(a["flags"]) | HEIGHT
                else:
                    du, a["p_up"] = up[0], up[1:]
                a["latitude"] = float(a["latitude"]) + dn / rn
                a["longitude"] = _wrap(float(a["longitude"]) + de / re)
                a["height_m"] = float(a["height_m"]) + du
                a["time"] = o["time"]
                a["n_applied"], a["run"], a["outliers_run"] = _inc(a["n_applied"]), _inc(a["run"]), 0
    if start:
        _start(c, a, o)
        flags |= INIT
    a["flags"] = (int(a["flags"]) & ~VELOCITY) | (VELOCITY if int(a["run"]) >= c["min_run"] else 0)
    f["latitude"], f["longitude"], f["height_m"], f["nis"], f["flags"] = a["latitude"], a["longitude"], a["height_m"], nis, flags
    return a, f


def apply(c, state, icaos, fixes, times, untracked=None, operands=None, step_fn=step, operand_fn=operand):
    """One update given fixes into state {icao: RECORD_DTYPE scalar}, in list order -> (FRAME_DTYPE per frame in list
    order, OPERAND_DTYPE per frame in list order).  Every tracked frame admits its aircraft.  operands: use these (list
    order) instead of computing them; step_fn / operand_fn: the model's, or functions of the same arguments built on the
    CPU mirror."""
    frames = np.zeros(len(icaos), dtype=FRAME_DTYPE)
    ops = np.zeros(len(icaos), dtype=OPERAND_DTYPE)
    for k, icao in enumerate(icaos):
        if untracked is not None and untracked[k]:
            continue
        icao = int(icao)
        ops[k] = operand_fn(c, fixes[k], float(times[k])) if operands is None else operands[k]
        state[icao], frames[k] = step_fn(c, state.get(icao, empty()), ops[k])
    return frames, ops


def sorted_order(icaos):
    """The list indices in the device's sorted order: ascending address, list order within one."""
    return np.argsort(np.asarray(icaos, dtype=np.int64), kind="stable")


def records(state, icaos):
    out = np.zeros(len(icaos), dtype=RECORD_DTYPE)
    for k, icao in enumerate(icaos):
        out[k] = state.get(int(icao), empty())
    return out


def rel_diff(got, want):
    """The largest |got - want| / max(|got|, |want|, 1) over two float arrays (1 unit of the field as the floor, so a
    value near zero counts by its absolute error); equal NaNs and equal infinities differ by 0."""
    got, want = np.asarray(got, dtype=np.float64).ravel(), np.asarray(want, dtype=np.float64).ravel()
    if got.size == 0:
        return 0.0
    same = (got == want) | (np.isnan(got) & np.isnan(want))
    with np.errstate(invalid="ignore"):
        d = np.abs(got - want) / np.maximum(np.maximum(np.abs(got), np.abs(want)), 1.0)
    d[same] = 0.0
    d[np.isnan(d)] = np.inf
    return float(d.max())


def compare(got, want, exact, f64, f32, what=""):
    """Exact fields equal, f32 fields equal or neighbours; -> the largest rel_diff over the f64 fields."""
    assert len(got) == len(want) and got.dtype.itemsize == want.dtype.itemsize, (what, len(got), len(want))
    for name in exact:
        same = got[name] == want[name]
        if got[name].dtype.kind == "f":
            same |= np.isnan(got[name]) & np.isnan(want[name])
        assert same.all(), (what, name, np.nonzero(~same.reshape(len(got), -1).all(axis=1))[0][:5])
    for name in f32:
        g, w = got[name].astype(np.float32), want[name].astype(np.float32)
        near = np.abs(g.astype(np.float64) - w.astype(np.float64)) <= np.spacing(np.abs(w)).astype(np.float64)
        assert near.all(), (what, name, np.nonzero(~near)[0][:5])
    return max([rel_diff(got[name], want[name]) for name in f64] + [0.0])


def compare_records(got, want, what=""):
    return compare(got, want, RECORD_EXACT, RECORD_F64, RECORD_F32, what)


def compare_frames(got, want, what=""):
    return compare(got, want, FRAME_EXACT, FRAME_F64, FRAME_F32, what)


def compare_operands(got, want, what=""):
    return compare(got, want, OPERAND_EXACT, OPERAND_F64, (), what)
