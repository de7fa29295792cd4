"""An exact check of what a multilaterate fix CLAIMS, from the inputs alone (mpmath, 50 digits).  It knows nothing of the
solver: no starting point, no damping, no step rule, no order of summation.  Given the receivers, the used receptions of
one message and the cfg, a reported fix (latitude, longitude, height_m, time_s, residual_rms_m, pdop, hdop, vdop) is held
to what those numbers mean in include/adsb_hip.h, "Multilaterate":

  rho_k        = c x (dt_k x seconds_per_tick - (clock_k - clock_0)), dt_k the integer time difference to the first
                 used reception (mod 2^48 for ticks, mod 2^64 for reception times, taken as signed), every factor the
                 exact value of its f64
  p, d         = the ECEF point of the reported latitude, longitude and height on WGS-84, and time_s x c
  rows         = range_k(p) + d - rho_k per used reception, and h(p) - the decoded altitude when the fix is ALTITUDE,
                 h the exact geodetic height (fixed-point iteration to 45 digits, not Bowring)
  residual     residual_rms_m is the rms of the rows
  time         d = mean(rho_k - range_k(p)): the d-equation of the least-squares point, sum(range_k + d - rho_k) = 0
  stationary   the undamped Gauss-Newton step -(Jt J)^-1 Jt r at (p, d) is short
  dilutions    pdop, hdop, vdop are the square roots of the trace, the east + north part and the up part of the position
               block of (Jt J)^-1, east / north / up taken at p's exact geodetic latitude and longitude
  height       a VALID ALTITUDE fix of 3 receivers has 4 rows and 4 unknowns; the altitude row's square cannot exceed
               the sum 4 rms^2, so |height_m - altitude| <= 2 rms (derived; (1 + 1e-6) and the floor for the f32 of rms)

The bounds on time, step and dilutions cannot be derived: they are measured on the numpy model's own fixes (never on the
library's) over the case lists and the edge lists of tests/mlat_cases.py, and 10 x the largest value is the tolerance,
for the order of summation (profiles/mlat_edges_checks.txt; tests/test_mlat_exact.py prints them again)."""
import mpmath as mp
import numpy as np

from tests import mlat_model as M          # record layouts, flag bits, the measured tolerances of the rms; not the solver

DIGITS = 50
# measured on the model's VALID fixes with pdop <= 20 (profiles/mlat_edges_checks.txt)
MODEL_MEASURED = {"time_s": 9.7e-16, "step_m": 1.7e-4, "pdop": 5.3e-8, "hdop": 5.1e-8, "vdop": 5.7e-8}
TOL = {k: 10 * v for k, v in MODEL_MEASURED.items()}


def _f(v):
    return mp.mpf(float(v))


def _wgs84():
    a, f = mp.mpf(6378137), 1 / mp.mpf("298.257223563")
    return a, f * (2 - f)


def ecef_of(lat_deg, lon_deg, h):
    """The exact ECEF point of three f64 (degrees, degrees, metres)."""
    a, e2 = _wgs84()
    phi, lam, h = _f(lat_deg) * mp.pi / 180, _f(lon_deg) * mp.pi / 180, _f(h)
    n = a / mp.sqrt(1 - e2 * mp.sin(phi) ** 2)
    return [(n + h) * mp.cos(phi) * mp.cos(lam), (n + h) * mp.cos(phi) * mp.sin(lam), (n * (1 - e2) + h) * mp.sin(phi)]


def geodetic_of(p):
    """(height, phi, lambda) of an ECEF point: phi = atan2(z + e2 N(phi) sin phi, P) iterated until it stands still."""
    a, e2 = _wgs84()
    x, y, z = p
    P = mp.sqrt(x * x + y * y)
    phi = mp.atan2(z, P * (1 - e2))
    for _ in range(200):
        n = a / mp.sqrt(1 - e2 * mp.sin(phi) ** 2)
        nxt = mp.atan2(z + e2 * n * mp.sin(phi), P)
        done = abs(nxt - phi) < mp.mpf(10) ** -(DIGITS - 5)
        phi = nxt
        if done:
            break
    else:
        raise AssertionError("the latitude iteration did not converge")
    h = P * mp.cos(phi) + z * mp.sin(phi) - a * mp.sqrt(1 - e2 * mp.sin(phi) ** 2)
    return h, phi, mp.atan2(y, x)


def altitude_of(b):
    """Metres (exact) or None: DF17/18, type code 9-18, a non-zero 12-bit code with the Q bit; 25 ft steps from -1000 ft."""
    if int(b[0]) >> 3 not in (17, 18) or not 9 <= int(b[4]) >> 3 <= 18:
        return None
    code = int(b[5]) << 4 | int(b[6]) >> 4
    if code == 0 or not code & 0x10:
        return None
    return (((code >> 5) << 4 | (code & 0xF)) * 25 - 1000) * mp.mpf("0.3048")


def used_of(msg, recs, rx, time_source):
    """(receiver indices, integer times) of a message's used receptions: the first reception of each receiver."""
    mine = recs[int(msg["first"]):int(msg["first"]) + int(msg["n_receptions"])]
    seen, who, when = set(), [], []
    for r in mine:
        if int(r["receiver"]) in seen:
            continue
        seen.add(int(r["receiver"]))
        who.append(int(r["receiver"]))
        when.append(int(rx["ticks"][int(r["frame"])]) if time_source == M.TIME_TICKS else int(r["time"]))
    return who, when


def rho_of(receivers, who, when, time_source, seconds_per_tick):
    """The exact rho_k from the integer times, the declared offsets and c."""
    bits = 48 if time_source == M.TIME_TICKS else 64
    out = []
    for k, t in zip(who, when):
        dt = ((t - when[0]) % (1 << bits) + (1 << bits - 1)) % (1 << bits) - (1 << bits - 1)
        out.append(_f(M.C_AIR) * (dt * _f(seconds_per_tick) - (_f(receivers["clock_offset_s"][k]) -
                                                                 _f(receivers["clock_offset_s"][who[0]]))))
    return out


def figures(stations, rho, altitude, fix):
    """What the fix claims against the exact values, as plain floats: rms_exact, rms (the reported one), time_s (the gap
    of time_s to mean(rho - range) / c), step_m, the relative gaps pdop / hdop / vdop, and height_gap_m (ALTITUDE only).
    stations: exact ECEF points of the used receivers; rho: their exact rho; altitude: the decoded one (exact) when the
    fix is ALTITUDE, else None."""
    with mp.workdps(DIGITS):
        c = _f(M.C_AIR)
        p = ecef_of(fix["latitude"], fix["longitude"], fix["height_m"])
        d = _f(fix["time_s"]) * c
        h, phi, lam = geodetic_of(p)
        rows, res, ranges = [], [], []
        for s, r in zip(stations, rho):
            diff = [p[i] - s[i] for i in range(3)]
            rng = mp.sqrt(sum(v * v for v in diff))
            ranges.append(rng)
            rows.append([v / rng for v in diff] + [mp.mpf(1)])
            res.append(rng + d - r)
        up = [mp.cos(phi) * mp.cos(lam), mp.cos(phi) * mp.sin(lam), mp.sin(phi)]
        if altitude is not None:
            rows.append(up + [mp.mpf(0)])
            res.append(h - altitude)
        J, r = mp.matrix(rows), mp.matrix(res)
        N = J.T * J
        inv = N ** -1
        step = -(inv * (J.T * r))
        east = mp.matrix([-mp.sin(lam), mp.cos(lam), 0])
        north = mp.matrix([-mp.sin(phi) * mp.cos(lam), -mp.sin(phi) * mp.sin(lam), mp.cos(phi)])
        Q = inv[0:3, 0:3]
        q = lambda v: (v.T * Q * v)[0]
        exact = {"pdop": mp.sqrt(Q[0, 0] + Q[1, 1] + Q[2, 2]), "hdop": mp.sqrt(q(east) + q(north)),
                 "vdop": mp.sqrt(q(mp.matrix(up)))}
        mean = sum(a - b for a, b in zip(rho, ranges)) / len(rho)
        out = {"rms_exact": float(mp.sqrt(sum(v * v for v in res) / len(res))), "rms": float(fix["residual_rms_m"]),
               "time_s": float(abs(d - mean) / c), "step_m": float(mp.sqrt(sum(step[i] ** 2 for i in range(3))))}
        for k, v in exact.items():
            out[k] = float(abs(_f(fix[k]) - v) / v)
        if altitude is not None:
            out["height_gap_m"] = float(abs(_f(fix["height_m"]) - altitude))
        out["rows"] = len(res)
        return out


def figures_of(receivers, msg, recs, rx, cfg, fix):
    """figures() of one message of a correlate result under the keywords of host_multilaterate / multilaterate_of."""
    src = cfg.get("time_source", M.TIME_RECEPTION)
    src = {"reception": M.TIME_RECEPTION, "ticks": M.TIME_TICKS}.get(src, src)
    spt = cfg.get("seconds_per_tick") or 1.0 / 12e6
    with mp.workdps(DIGITS):
        who, when = used_of(msg, recs, rx, src)
        assert len(who) == int(fix["n_used"])
        stations = [ecef_of(receivers["latitude"][k], receivers["longitude"][k], receivers["height_m"][k]) for k in who]
        altitude = altitude_of(msg["bytes"]) if int(fix["flags"]) & M.ALTITUDE else None
        assert (altitude is not None) == bool(int(fix["flags"]) & M.ALTITUDE)
        return figures(stations, rho_of(receivers, who, when, src, spt), altitude, fix)


def broken(fig, n_used, valid=True):
    """The claims a fix does not keep, as a list of (what, figure, bound); empty: the fix is what it says."""
    bad = []
    rms_rel = M.MIRROR_VS_MODEL_TOL["residual_rms_m"]
    if abs(fig["rms"] - fig["rms_exact"]) > M.RMS_FLOOR_M + rms_rel * fig["rms_exact"]:
        bad.append(("residual_rms_m", fig["rms"], fig["rms_exact"]))
    for k in ("time_s", "step_m", "pdop", "hdop", "vdop"):
        if not fig[k] <= TOL[k]:
            bad.append((k, fig[k], TOL[k]))
    if valid and "height_gap_m" in fig and n_used == 3:
        bound = 2 * fig["rms"] * (1 + 1e-6) + M.RMS_FLOOR_M
        if not fig["height_gap_m"] <= bound:
            bad.append(("height_m", fig["height_gap_m"], bound))
    return bad


def check_list(name, receivers, lst, cfg, fixes, worst=None):
    """Every VALID fix of a list with pdop <= 20 keeps its claims.  worst (a dict) takes the largest figure per
    bound.  -> the number of fixes checked."""
    n = 0
    for g, fix in enumerate(fixes):
        if not int(fix["flags"]) & M.VALID or not fix["pdop"] <= 20:
            continue
        fig = figures_of(receivers, lst["msgs"][g], lst["recs"], lst["rx"], cfg, fix)
        n += 1
        if worst is not None:
            for k in TOL:
                worst[k] = max(worst.get(k, 0.0), fig[k])
            over = max(abs(fig["rms"] - fig["rms_exact"]) - M.RMS_FLOOR_M, 0.0) / max(fig["rms_exact"], M.RMS_FLOOR_M)
            worst["residual_rms_m"] = max(worst.get("residual_rms_m", 0.0), over)
        assert not broken(fig, int(fix["n_used"])), (name, g, broken(fig, int(fix["n_used"])))
    return n
