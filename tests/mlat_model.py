"""An independent numpy restatement of include/adsb_hip.h, "Multilaterate": it calls no library entry point.

One message at a time: the used rule, the integer time differences, rho, the two-stage Levenberg-Marquardt solve with
the header's step rule and L D Lt pivot rule, Bowring's height with two refinement steps, the dilutions and the flags.
The sums over receptions are numpy's (J.T @ J), NOT the header's 16-partial butterfly, so positions agree with the
library to a tolerance and not to the bit; the tolerance is measured (see MIRROR_VS_MODEL_TOL_M below)."""
import math

import numpy as np

MESSAGE_DTYPE = np.dtype([("time", "<u8"), ("bytes", "u1", (14,)), ("status", "u1"), ("fixed_bit", "u1"), ("first", "<u4"),
                          ("n_receptions", "<u4"), ("n_receivers", "<u2"), ("first_receiver", "<u2"),
                          ("best_receiver", "<u2"), ("reserved", "<u2"), ("n_clean", "<u4"), ("reserved2", "<u4"),
                          ("span", "<u8"), ("best_signal_sum", "<u8")])
RECEPTION_DTYPE = np.dtype([("time", "<u8"), ("frame", "<u4"), ("receiver", "<u2"), ("reserved", "<u2")])
WIRE_RX_DTYPE = np.dtype([("ticks", "<u8"), ("pos", "<u4"), ("signal", "u1"), ("kind", "u1"), ("receiver", "<u2")])
RECEIVER_DTYPE = np.dtype([("latitude", "<f8"), ("longitude", "<f8"), ("height_m", "<f8"), ("clock_offset_s", "<f8")])
FIX_DTYPE = np.dtype([("latitude", "<f8"), ("longitude", "<f8"), ("height_m", "<f8"), ("time_s", "<f8"),
                      ("residual_rms_m", "<f4"), ("pdop", "<f4"), ("hdop", "<f4"), ("vdop", "<f4"), ("n_used", "<u2"),
                      ("iterations", "<u2"), ("flags", "<u4"), ("reserved", "<u8")])

C_AIR = 299792458.0 / 1.0003
MAX_RECEPTIONS = 256
TIME_RECEPTION, TIME_TICKS = 0, 1
ATTEMPTED, CONVERGED, ALTITUDE, TOO_FEW, TOO_MANY, SINGULAR = 0x1, 0x2, 0x4, 0x8, 0x10, 0x20
REJECTED_RESIDUAL, REJECTED_RANGE, VALID, BAD_INDEX = 0x40, 0x80, 0x100, 0x200
A, F = 6378137.0, 1.0 / 298.257223563
B = A * (1.0 - F)
E2 = F * (2.0 - F)
EP2 = (A * A - B * B) / (B * B)

# Measured on the case lists of tests/mlat_cases.py (profiles/mlat_checks.txt): the largest distance between the
# mirror's and this model's position over fixes with pdop <= 20 was 6.3e-5 m; the tolerance is 10 x that, because this
# model sums in numpy's order and not in the butterfly's.
MIRROR_VS_MODEL_MEASURED_M = 6.3e-5
MIRROR_VS_MODEL_TOL_M = 10 * MIRROR_VS_MODEL_MEASURED_M

# The other fields of a fix, measured the same way over the case lists and the edge lists of tests/mlat_cases.py
# (profiles/mlat_edges_checks.txt), over fixes with equal integers and pdop <= 20; each tolerance is 10 x the measured gap.
#   hdop, vdop             relative
#   time_s, height_m       absolute, seconds and metres
#   residual_rms_m         relative above RMS_FLOOR_M: |a - b| <= RMS_FLOOR_M + rel x the reference's
# RMS_FLOOR_M is derived, not measured.  A coordinate of the point is about 6.4e6 m, which an f64 holds to 6.4e6 x 2^-52
# = 1.4e-9 m, so no residual of a range row (range + d - rho, the range taken from three such coordinates) is known
# more finely than a few of these steps however the sums are ordered.  Where a fix is exactly determined (4 free
# receivers, or 3 and the altitude) the rms is nothing but that noise, plus the s^2 / (2 range) < 1e-9 m that a last step
# s < 0.01 m leaves undone, and two summation orders differ in it by factors.  16 steps cover the three coordinates,
# the up to five rows of such a fix and that remainder: 16 x 6.4e6 x 2^-52 = 2.3e-8 m.
RMS_FLOOR_M = 16 * 6.4e6 * 2.0 ** -52
MIRROR_VS_MODEL_MEASURED = {"hdop": 0.0, "vdop": 0.0, "time_s": 2.1e-13, "height_m": 3.2e-6, "residual_rms_m": 0.0}
# hdop, vdop and residual_rms_m are f32, and mirror and model gave the same f32 everywhere: measured 0.  Ten times
# nothing would demand equal bits of two f64 results that may differ in their last places, which the rounding to f32
# turns into one step of that format; so their tolerance is never below that step, 2^-23.
F32_STEP = 2.0 ** -23
MIRROR_VS_MODEL_TOL = {k: max(10 * v, F32_STEP) if k in ("hdop", "vdop", "residual_rms_m") else 10 * v
                       for k, v in MIRROR_VS_MODEL_MEASURED.items()}


def gaps_of(a, b):
    """{field: (gap, tolerance)} of fix a against the reference fix b, in the units above."""
    out = {}
    for k in ("hdop", "vdop"):
        out[k] = abs(float(a[k]) - float(b[k])) / float(b[k]) if b[k] > 0 else float(a[k] != b[k])
    for k in ("time_s", "height_m"):
        out[k] = abs(float(a[k]) - float(b[k]))
    rms = float(b["residual_rms_m"])
    over = abs(float(a["residual_rms_m"]) - rms) - RMS_FLOOR_M
    out["residual_rms_m"] = max(over, 0.0) / rms if rms > 0 else float(over > 0)
    return {k: (v, MIRROR_VS_MODEL_TOL[k]) for k, v in out.items()}


def ecef_of(lat_deg, lon_deg, h):
    phi, lam = math.radians(lat_deg), math.radians(lon_deg)
    n = A / math.sqrt(1.0 - E2 * math.sin(phi) ** 2)
    return np.array([(n + h) * math.cos(phi) * math.cos(lam), (n + h) * math.cos(phi) * math.sin(lam),
                     (n * (1.0 - E2) + h) * math.sin(phi)])


def geodetic_of(p):
    """(height, normal, phi, lambda) of an ECEF point: Bowring with two refinement steps."""
    x, y, z = (float(v) for v in p)
    P = math.hypot(x, y)
    cl, sl = (x / P, y / P) if P > 0 else (1.0, 0.0)
    beta = math.atan2(A * z, B * P)
    phi = 0.0
    for _ in range(2):
        phi = math.atan2(z + EP2 * B * math.sin(beta) ** 3, P - E2 * A * math.cos(beta) ** 3)
        beta = math.atan2(B * math.sin(phi), A * math.cos(phi))
    h = P * math.cos(phi) + z * math.sin(phi) - A * math.sqrt(1.0 - E2 * math.sin(phi) ** 2)
    return h, np.array([math.cos(phi) * cl, math.cos(phi) * sl, math.sin(phi)]), phi, math.atan2(sl, cl)


def altitude_of(b):
    """Metres, or None: DF17/18, type code 9-18, a non-zero altitude code with the Q bit."""
    df, tc = int(b[0]) >> 3, int(b[4]) >> 3
    if df not in (17, 18) or not 9 <= tc <= 18:
        return None
    code = int(b[5]) << 4 | int(b[6]) >> 4
    if code == 0 or not code & 0x10:
        return None
    return (((code >> 5) << 4 | (code & 0xF)) * 25 - 1000) * 0.3048


def _ldl_solve(M, rhs):
    """x of M x = rhs by L D Lt in the given order without pivoting; None when a pivot is not > 1e-12 x its diagonal."""
    n = len(M)
    Lm, D = np.eye(n), np.zeros(n)
    for j in range(n):
        d = M[j, j] - sum(Lm[j, k] ** 2 * D[k] for k in range(j))
        if not d > 1e-12 * M[j, j]:
            return None
        D[j] = d
        for i in range(j + 1, n):
            Lm[i, j] = (M[i, j] - sum(Lm[i, k] * Lm[j, k] * D[k] for k in range(j))) / d
    y = np.linalg.solve(Lm, rhs) / D
    return np.linalg.solve(Lm.T, y)


def _system(x, S, rho, height):
    """(J, r) of the stage's equations at x; height None: no altitude row."""
    d = x[:3] - S
    rng = np.sqrt((d * d).sum(axis=1))
    safe = np.where(rng > 0, rng, 1.0)
    J = np.hstack([np.where((rng > 0)[:, None], d / safe[:, None], 0.0), np.ones((len(S), 1))])
    r = rng + x[3] - rho
    if height is not None:
        h, nrm, _, _ = geodetic_of(x[:3])
        J = np.vstack([J, [nrm[0], nrm[1], nrm[2], 0.0]])
        r = np.append(r, h - height)
    return J, r


def _stage(x, S, rho, height, max_it, tol):
    """-> (x, J, r, steps taken, converged, singular, last step length)"""
    J, r = _system(x, S, rho, height)
    lam, last = 1e-3, float("nan")
    for it in range(max_it):
        N = J.T @ J
        M = N + lam * np.diag(np.diag(N))
        delta = _ldl_solve(M, -(J.T @ r))
        if delta is None:
            return x, J, r, it, False, True, last
        Jt, rt = _system(x + delta, S, rho, height)
        last = float(np.sqrt((delta[:3] ** 2).sum()))
        if (rt * rt).sum() <= (r * r).sum():
            x, J, r = x + delta, Jt, rt
            lam = max(lam / 10.0, 1e-12)
        else:
            lam = min(lam * 10.0, 1e12)
        if last < tol:
            return x, J, r, it + 1, True, False, last
    return x, J, r, max_it, False, False, last


def multilaterate(receivers, msgs, recs, rx=None, time_source=TIME_RECEPTION, seconds_per_tick=0.0, use_altitude=False,
                  min_receivers=0, max_iterations=0, step_tol_m=0.0, max_residual_m=0.0, max_range_m=0.0,
                  default_altitude_m=0.0):
    """-> (fixes, header dict, last step length per message (nan where none))"""
    receivers = np.asarray(receivers, dtype=RECEIVER_DTYPE)
    st = np.array([ecef_of(r["latitude"], r["longitude"], r["height_m"]) for r in receivers]).reshape(-1, 3)
    clk = receivers["clock_offset_s"].astype(np.float64)
    spt = seconds_per_tick or 1.0 / 12e6
    max_it, tol = max_iterations or 24, step_tol_m or 0.01
    max_range, h_default = max_range_m or 500e3, default_altitude_m or 10000.0
    fixes = np.zeros(len(msgs), dtype=FIX_DTYPE)
    lasts = np.full(len(msgs), np.nan)
    for g, m in enumerate(msgs):
        n, first = int(m["n_receptions"]), int(m["first"])
        if first + n > len(recs):
            fixes[g]["flags"] = BAD_INDEX
            continue
        if n > MAX_RECEPTIONS:
            fixes[g]["flags"] = TOO_MANY
            continue
        mine = recs[first:first + n]
        if (mine["receiver"] >= len(receivers)).any() or (time_source == TIME_TICKS and (mine["frame"] >= len(rx)).any()):
            fixes[g]["flags"] = BAD_INDEX
            continue
        seen, used = set(), []
        for k in range(n):
            if int(mine["receiver"][k]) not in seen:
                seen.add(int(mine["receiver"][k]))
                used.append(k)
        alt = altitude_of(m["bytes"]) if use_altitude else None
        need = max(min_receivers, 3 if alt is not None else 4)
        fixes[g]["n_used"] = len(used)
        if len(used) < need:
            fixes[g]["flags"] = TOO_FEW
            continue
        rcv = mine["receiver"][used].astype(int)
        t = [int(rx["ticks"][int(j)]) for j in mine["frame"][used]] if time_source == TIME_TICKS else \
            [int(v) for v in mine["time"][used]]
        if time_source == TIME_TICKS:
            dt = [((v - t[0]) % (1 << 48) + (1 << 47)) % (1 << 48) - (1 << 47) for v in t]
        else:
            dt = [((v - t[0]) % (1 << 64) + (1 << 63)) % (1 << 64) - (1 << 63) for v in t]
        rho = C_AIR * (np.array([float(v) for v in dt]) * spt - (clk[rcv] - clk[rcv[0]]))
        S = st[rcv]
        cen = S.sum(axis=0) / len(used)
        hc, nc, _, _ = geodetic_of(cen)
        height = alt if alt is not None else h_default
        p0 = cen + nc * (height - hc)
        x = np.append(p0, -math.sqrt(((p0 - S[0]) ** 2).sum()))
        x, J, r, its, conv, sing, last = _stage(x, S, rho, height, max_it, tol)
        if alt is None and not sing:
            x, J, r, it2, conv, sing, last = _stage(x, S, rho, None, max_it, tol)
            its += it2
        flags = ATTEMPTED | (ALTITUDE if alt is not None else 0)
        f = fixes[g]
        h, nrm, phi, lam = geodetic_of(x[:3])
        if not sing:
            N = J.T @ J
            cols = [_ldl_solve(N, e) for e in np.eye(4)[:3]]
            if cols[0] is None:
                sing = True
            else:
                Q = np.array(cols)[:, :3]
                east = np.array([-math.sin(lam), math.cos(lam), 0.0])
                north = np.array([-math.sin(phi) * math.cos(lam), -math.sin(phi) * math.sin(lam), math.cos(phi)])
                f["pdop"] = math.sqrt(np.trace(Q))
                f["hdop"] = math.sqrt(max(east @ Q @ east + north @ Q @ north, 0.0))
                f["vdop"] = math.sqrt(max(nrm @ Q @ nrm, 0.0))
        f["latitude"], f["longitude"], f["height_m"] = math.degrees(phi), math.degrees(lam), h
        f["time_s"] = x[3] / C_AIR
        rms = math.sqrt((r * r).sum() / len(r))
        f["residual_rms_m"] = rms
        f["iterations"] = its
        flags |= (CONVERGED if conv else 0) | (SINGULAR if sing else 0)
        if max_residual_m > 0 and not rms <= max_residual_m:
            flags |= REJECTED_RESIDUAL
        if not math.sqrt(((x[:3] - cen) ** 2).sum()) <= max_range:
            flags |= REJECTED_RANGE
        if conv and not flags & (SINGULAR | REJECTED_RESIDUAL | REJECTED_RANGE):
            flags |= VALID
        f["flags"] = flags
        lasts[g] = last
    header = {"n_messages": len(msgs), "n_attempted": int((fixes["flags"] & ATTEMPTED != 0).sum()),
              "n_valid": int((fixes["flags"] & VALID != 0).sum()), "flags": int((fixes["flags"] & BAD_INDEX != 0).any())}
    return fixes, header, lasts


def position_gap_m(a, b):
    """ECEF distance between two fixes' positions."""
    return float(np.sqrt(((ecef_of(a["latitude"], a["longitude"], a["height_m"]) -
                           ecef_of(b["latitude"], b["longitude"], b["height_m"])) ** 2).sum()))
