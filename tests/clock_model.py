"""An independent numpy restatement of include/adsb_hip.h, "Clock sync": it calls no library entry point.

The rows are built as plain Python (the used rule, the integer tick differences, the single-message position decode of
tests/fix_model.py, numpy ECEF and ranges), the reached set is a breadth-first walk, and the unknowns are solved with
numpy.linalg.lstsq over the rows themselves -- NOT the header's pair sums, normal equations and L D Lt -- so offsets and
drifts agree with the library to a tolerance and not to the bit; the tolerance is measured (MIRROR_VS_MODEL_* below)."""
import math

import numpy as np

from tests import fix_model as F
from tests import mlat_model as M

CLOCK_DTYPE = np.dtype([("offset_s", "<f8"), ("fine_offset_s", "<f8"), ("drift", "<f8"), ("residual_rms_s", "<f4"),
                        ("n_rows", "<u4"), ("n_dropped", "<u4"), ("n_partners", "<u4"), ("flags", "<u4"),
                        ("reserved", "<u4", (5,))])
DRIFT = 0x1
REFERENCE, REACHED, HAS_DRIFT = 0x1, 0x2, 0x4
HDR_BAD_INDEX, HDR_DRIFT_DROPPED, HDR_SINGULAR = 0x1, 0x2, 0x4
INTEGER_FIELDS = ("n_rows", "n_dropped", "n_partners", "flags")

# Measured on the case lists of tests/clock_cases.py (profiles/clock_checks.txt): the largest difference between the
# mirror's and this model's fine offset was 3.8e-15 s and between their drifts 1.7e-16 s/s (both on the 256-receiver
# list; 7.5e-17 s and 7.2e-18 s/s on the others); the tolerances are 10 x those, because this model solves the rows with lstsq (an SVD) and the mirror the
# normal equations of the pair sums.
MIRROR_VS_MODEL_MEASURED_S, MIRROR_VS_MODEL_MEASURED_DRIFT = 3.8e-15, 1.7e-16
MIRROR_VS_MODEL_TOL_S, MIRROR_VS_MODEL_TOL_DRIFT = 10 * MIRROR_VS_MODEL_MEASURED_S, 10 * MIRROR_VS_MODEL_MEASURED_DRIFT
# Device against mirror: the same operations in the same order, but for the last bit of sin / cos / sqrt in the decode, the
# ECEF point and the ranges.  Measured on the same lists on an MI355X (profiles/clock_checks.txt): 7.4e-18 s on the
# 33-receiver list and 1.1e-18 s/s; 0 on the 256-receiver list.  The shape lists of tests/test_clock_host.py stayed
# under 8.7e-18 s and 2.9e-19 s/s.
DEVICE_VS_MIRROR_MEASURED_S, DEVICE_VS_MIRROR_MEASURED_DRIFT = 7.4e-18, 1.1e-18
DEVICE_VS_MIRROR_TOL_S, DEVICE_VS_MIRROR_TOL_DRIFT = 10 * DEVICE_VS_MIRROR_MEASURED_S, 10 * DEVICE_VS_MIRROR_MEASURED_DRIFT


def _signed(v, bits):
    return (v % (1 << bits) + (1 << (bits - 1))) % (1 << bits) - (1 << (bits - 1))


def _source(time_source):
    return {"reception": M.TIME_RECEPTION, "ticks": M.TIME_TICKS}.get(time_source, time_source)


def _times(time_source, seconds_per_tick, seconds_per_time):
    spt = seconds_per_tick or 1.0 / 12e6
    return spt, (seconds_per_time or spt), (48 if time_source == M.TIME_TICKS else 64)


def _raw(time_source, rec, rx):
    return int(rx["ticks"][int(rec["frame"])]) if time_source == M.TIME_TICKS else int(rec["time"])


def rows_of(receivers, msgs, recs, rx=None, time_source=M.TIME_RECEPTION, seconds_per_tick=0.0, seconds_per_time=0.0,
            max_range_nm=0.0, **_):
    """-> (rows as dicts {slot, i, j, tau, y, msg}, n_eligible, bad_index)"""
    receivers = np.asarray(receivers, dtype=M.RECEIVER_DTYPE)
    R, time_source = len(receivers), _source(time_source)
    st = np.array([M.ecef_of(r["latitude"], r["longitude"], r["height_m"]) for r in receivers]).reshape(-1, 3)
    prior = receivers["clock_offset_s"].astype(np.float64)
    spt, sptime, bits = _times(time_source, seconds_per_tick, seconds_per_time)
    rows, eligible, bad = [], 0, False
    for g, m in enumerate(msgs):
        n, first = int(m["n_receptions"]), int(m["first"])
        if first + n > len(recs):
            bad = True
            continue
        if n > M.MAX_RECEPTIONS:
            continue
        mine = recs[first:first + n]
        if (mine["receiver"] >= R).any() or (time_source == M.TIME_TICKS and (mine["frame"] >= len(rx)).any()):
            bad = True
            continue
        seen, used = set(), []
        for k in range(n):
            if int(mine["receiver"][k]) not in seen:
                seen.add(int(mine["receiver"][k]))
                used.append(k)
        if len(used) < 2 or M.altitude_of(m["bytes"]) is None:
            continue
        i = int(mine["receiver"][0])
        d = F.decode((float(receivers["latitude"][i]), float(receivers["longitude"][i]), max_range_nm or 180.0),
                     bytes(m["bytes"]))
        if d is None or d["flags"] & (F.VALID | F.SURFACE | F.ALT) != (F.VALID | F.ALT):
            continue
        eligible += 1
        p = M.ecef_of(d["latitude"], d["longitude"], d["altitude"] * 0.3048)
        tau = float(_signed(int(m["time"]) - int(msgs[0]["time"]), 64)) * sptime
        t0 = _raw(time_source, mine[0], rx)
        for k in used[1:]:
            j = int(mine["receiver"][k])
            dt = _signed(_raw(time_source, mine[k], rx) - t0, bits)
            y = float(dt) * spt - (prior[j] - prior[i]) - \
                (math.sqrt(((p - st[j]) ** 2).sum()) - math.sqrt(((p - st[i]) ** 2).sum())) / M.C_AIR
            rows.append({"slot": first + k, "i": i, "j": j, "tau": tau, "y": y, "msg": g})
    return rows, eligible, bad


def _solve(rows, R, reference, drift, min_rows):
    """One pass over `rows` -> (a[R], b[R], reached[R], edges as a set of (lo, hi), header flags, drift solved)"""
    count = {}
    for r in rows:
        pair = (min(r["i"], r["j"]), max(r["i"], r["j"]))
        count[pair] = count.get(pair, 0) + 1
    edges = {pair for pair, n in count.items() if n >= min_rows}
    reached, frontier = {reference}, [reference]
    while frontier:
        u = frontier.pop()
        for lo, hi in edges:
            for a, b in ((lo, hi), (hi, lo)):
                if a == u and b not in reached:
                    reached.add(b)
                    frontier.append(b)
    unknown = [r for r in range(R) if r in reached and r != reference]
    used = [r for r in rows if (min(r["i"], r["j"]), max(r["i"], r["j"])) in edges and r["i"] in reached]
    flags = 0
    a, b = np.zeros(R), np.zeros(R)

    def attempt(stride):
        col = {r: q * stride for q, r in enumerate(unknown)}
        A, y = np.zeros((len(used), len(unknown) * stride)), np.zeros(len(used))
        for q, r in enumerate(used):
            y[q] = r["y"]
            for rcv, sign in ((r["j"], 1.0), (r["i"], -1.0)):
                if rcv in col:
                    A[q, col[rcv]] += sign
                    if stride == 2:
                        A[q, col[rcv] + 1] += sign * r["tau"]
        if A.shape[1] == 0:
            return col, np.zeros(0)
        if len(used) == 0 or np.linalg.matrix_rank(A) < A.shape[1]:
            return col, None
        return col, np.linalg.lstsq(A, y, rcond=None)[0]

    stride = 2 if drift else 1
    col, x = attempt(stride)
    if x is None and stride == 2:
        flags |= HDR_DRIFT_DROPPED
        stride = 1
        col, x = attempt(stride)
    if x is None:
        flags |= HDR_SINGULAR
    else:
        for r, c in col.items():
            a[r] = x[c]
            if stride == 2:
                b[r] = x[c + 1]
    return a, b, reached, edges, flags, (x is not None and stride == 2)


def residual(r, a, b):
    return r["y"] - ((a[r["j"]] + b[r["j"]] * r["tau"]) - (a[r["i"]] + b[r["i"]] * r["tau"]))


def clock_sync(receivers, msgs, recs, rx=None, reference=0, drift=True, min_rows=0, max_residual_s=0.0, **times):
    """-> (CLOCK_DTYPE clocks, header dict, row state per reception slot: 0 empty, 1 kept, 2 dropped, the residuals of
    the first pass by slot)"""
    receivers = np.asarray(receivers, dtype=M.RECEIVER_DTYPE)
    R = len(receivers)
    rows, eligible, bad = rows_of(receivers, msgs, recs, rx, **times)
    a, b, reached, edges, flags, drifted = _solve(rows, R, reference, drift, min_rows or 1)
    state = np.zeros(len(recs), dtype=np.uint8)
    first_residual = {r["slot"]: residual(r, a, b) for r in rows}
    kept = rows
    if max_residual_s > 0:
        kept = [r for r in rows if not abs(residual(r, a, b)) > max_residual_s]
        a, b, reached, edges, flags, drifted = _solve(kept, R, reference, drift, min_rows or 1)
    for r in rows:
        state[r["slot"]] = 2
    for r in kept:
        state[r["slot"]] = 1
    clocks = np.zeros(R, dtype=CLOCK_DTYPE)
    for u in range(R):
        mine = [r for r in kept if u in (r["i"], r["j"])]
        c = clocks[u]
        c["offset_s"], c["fine_offset_s"], c["drift"] = receivers["clock_offset_s"][u] + a[u], a[u], b[u]
        c["n_rows"] = len(mine)
        c["n_dropped"] = len([r for r in rows if u in (r["i"], r["j"])]) - len(mine)
        c["n_partners"] = len([e for e in edges if u in e])
        c["residual_rms_s"] = math.sqrt(sum(residual(r, a, b) ** 2 for r in mine) / len(mine)) if mine else 0.0
        c["flags"] = (REFERENCE if u == reference else 0) | (REACHED if u in reached else 0) | \
            (HAS_DRIFT if drifted and u in reached and u != reference else 0)
    header = {"n_messages": len(msgs), "n_eligible": eligible, "n_rows": len(rows), "n_dropped": len(rows) - len(kept),
              "n_reached": len(reached), "flags": flags | (HDR_BAD_INDEX if bad else 0)}
    return clocks, header, state, first_residual


def apply(clocks, msgs, recs, rx=None, time_source=M.TIME_RECEPTION, seconds_per_tick=0.0, seconds_per_time=0.0, **_):
    """-> (corrected receptions, per reception: the distance of llrint's argument from the nearest half, inf where the
    reception keeps its raw time)"""
    time_source = _source(time_source)
    spt, sptime, bits = _times(time_source, seconds_per_tick, seconds_per_time)
    out = recs.copy()
    half = np.full(len(recs), np.inf)
    if len(msgs) == 0:
        return out, half
    m0, ref = msgs[0], 0
    if int(m0["n_receptions"]) and int(m0["first"]) + int(m0["n_receptions"]) <= len(recs):
        r = recs[int(m0["first"])]
        if time_source != M.TIME_TICKS or int(r["frame"]) < len(rx):
            ref = _raw(time_source, r, rx)
    for m in msgs:
        n, first = int(m["n_receptions"]), int(m["first"])
        if first + n > len(recs):
            continue
        tau = float(_signed(int(m["time"]) - int(m0["time"]), 64)) * sptime
        for s in range(first, first + n):
            r = recs[s]
            u = int(r["receiver"])
            if u >= len(clocks) or (time_source == M.TIME_TICKS and int(r["frame"]) >= len(rx)):
                continue
            d = _signed(_raw(time_source, r, rx) - ref, bits)
            x = 256.0 * (float(clocks["offset_s"][u]) + float(clocks["drift"][u]) * tau) / spt
            out["time"][s] = (256 * d - int(round(x))) % (1 << 64)
            half[s] = abs(abs(x - math.floor(x)) - 0.5)
    return out, half
