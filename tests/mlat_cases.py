"""Scenarios for the multilaterate tests: receivers on rings around (47.45, 8.56), emitters out to 150 km, every message
a real DF17 airborne-position frame, reception ticks from exact ECEF distances -- built straight into a correlate
result (MESSAGE_DTYPE, RECEPTION_DTYPE, with the WIRE_RX_DTYPE records of TIME_TICKS beside it), and the small
hand-made lists of the edge tests."""
import math

import numpy as np

from tests import mlat_model as M
from tests import traffic

LAT0, LON0 = 47.45, 8.56
FRAME_DTYPE = np.dtype([("offset", "<u8"), ("bytes", "u1", (14,)), ("status", "u1"), ("fixed_bit", "u1")])
SPT_NS = 1e-9


def _offset(lat0, lon0, east, north):
    """Degrees of a point east / north metres from (lat0, lon0): good enough to place things.  A longitude past the
    antimeridian comes back into [-180, 180)."""
    lat, lon = lat0 + north / 111200.0, lon0 + east / (111200.0 * math.cos(math.radians(lat0)))
    if lon >= 180.0:
        lon -= 360.0
    elif lon < -180.0:
        lon += 360.0
    return lat, lon


def receivers(n, seed, clock_offsets=None, centre=(LAT0, LON0)):
    """n receivers on rings of 36-60 km radius around `centre`, at heights of 300-1800 m, spread in azimuth."""
    rng = np.random.default_rng(seed)
    out = np.zeros(n, dtype=M.RECEIVER_DTYPE)
    for k in range(n):
        az = 2 * math.pi * (k + rng.uniform(-0.25, 0.25)) / n
        rad = rng.uniform(36e3, 60e3)
        lat, lon = _offset(centre[0], centre[1], rad * math.sin(az), rad * math.cos(az))
        out[k] = (lat, lon, rng.uniform(300.0, 1800.0), 0.0 if clock_offsets is None else clock_offsets[k])
    return out


def altitude_code(height_m):
    """(12-bit altitude code with the Q bit, the height it decodes to) nearest to height_m."""
    n = int(round((height_m / 0.3048 + 1000.0) / 25.0))
    return (n >> 4) << 5 | 0x10 | (n & 0xF), (n * 25 - 1000) * 0.3048


def emitters(oracle, n, seed, max_range=150e3, centre=(LAT0, LON0)):
    """n emitters 0-150 km out from `centre` at 3-12 km: (ECEF positions, their frames).  Each height is one its frame's altitude code
    decodes to exactly, so the altitude equation is consistent with the truth."""
    rng = np.random.default_rng(seed)
    pos, frames = [], []
    for i in range(n):
        az, rad = rng.uniform(0, 2 * math.pi), max_range * math.sqrt(rng.uniform(0, 1))
        code, h = altitude_code(rng.uniform(3000.0, 12000.0))
        lat, lon = _offset(centre[0], centre[1], rad * math.sin(az), rad * math.cos(az))
        pos.append(M.ecef_of(lat, lon, h))
        frames.append(traffic.position_frame(oracle, 0x400000 + i, i & 1, int(rng.integers(0, 1 << 17)),
                                             int(rng.integers(0, 1 << 17)), alt_code=code, tc=11))
    return np.array(pos), frames


def build(rcv, pos, frames, spt=SPT_NS, heard=None, tick_base=0, spacing_s=2e-3, mod48=False, extra=None,
          offset_ticks=None):
    """A correlate result of emitter i heard by the receivers heard[i] (None: all): reception ticks = floor((emission +
    distance / c + the receiver's clock offset) / spt) + tick_base.  extra: (message, receiver, ticks later) triples, a
    second reception by a receiver that already has one.  offset_ticks: whole ticks added per receiver (a clock offset
    that is exact in ticks).  -> dict(msgs, recs, rx, frames, counts): receptions in (T, j) order inside a message, j the
    index in the receiver-major frame list `frames` (offset = T, counts[r] frames of receiver r), rx[j].ticks = T (mod
    2^48 with mod48)."""
    st = np.array([M.ecef_of(r["latitude"], r["longitude"], r["height_m"]) for r in rcv])
    rows = []                                               # (message, receiver, T)
    for i, p in enumerate(pos):
        for r in (range(len(rcv)) if heard is None else heard[i]):
            dist = math.sqrt(((p - st[r]) ** 2).sum())
            t = (i + 1) * spacing_s + dist / M.C_AIR + float(rcv["clock_offset_s"][r])
            rows.append((i, r, int(math.floor(t / spt)) + tick_base + (int(offset_ticks[r]) if offset_ticks is not None else 0)))
    for i, r, later in (extra or ()):
        t0 = [t for (a, b, t) in rows if a == i and b == r][0]
        rows.append((i, r, t0 + later))
    order = sorted(range(len(rows)), key=lambda k: (rows[k][1], rows[k][2]))        # receiver-major, ascending T
    frame_of = {k: j for j, k in enumerate(order)}
    rx = np.zeros(len(rows), dtype=M.WIRE_RX_DTYPE)
    for k, j in frame_of.items():
        rx[j] = (rows[k][2] % (1 << 48) if mod48 else rows[k][2], 0, 0, ord("3"), rows[k][1])
    flist = np.zeros(len(rows), dtype=FRAME_DTYPE)
    for k, j in frame_of.items():
        flist[j] = (rows[k][2] % (1 << 64), np.frombuffer(frames[rows[k][0]], dtype=np.uint8), 0, 0xFF)
    counts = np.bincount([row[1] for row in rows], minlength=len(rcv)).astype(np.uint64)
    msgs = np.zeros(len(pos), dtype=M.MESSAGE_DTYPE)
    recs = np.zeros(len(rows), dtype=M.RECEPTION_DTYPE)
    of_msg = {}
    for k, row in enumerate(rows):
        of_msg.setdefault(row[0], []).append(k)
    at = 0
    for i in range(len(pos)):
        mine = sorted(of_msg.get(i, []), key=lambda k: (rows[k][2], frame_of[k]))
        for q, k in enumerate(mine):
            recs[at + q] = (rows[k][2] % (1 << 64), frame_of[k], rows[k][1], 0)
        m = msgs[i]
        m["bytes"] = np.frombuffer(frames[i], dtype=np.uint8)
        m["first"], m["n_receptions"] = at, len(mine)
        m["fixed_bit"] = 0xFF
        if mine:
            m["time"] = recs[at]["time"]
            m["span"] = recs[at + len(mine) - 1]["time"] - recs[at]["time"]
            m["first_receiver"] = recs[at]["receiver"]
            m["n_receivers"] = len(set(rows[k][1] for k in mine))
        m["best_receiver"] = 0xFFFF
        m["n_clean"] = len(mine)
        at += len(mine)
    return {"msgs": msgs, "recs": recs, "rx": rx, "frames": flist, "counts": counts}


# the truth lists: (name, receivers, use_altitude, the issue's numpy experiment's largest 3-D error for the row)
TRUTH_ROWS = (("6 receivers free", 6, False, 20.6), ("8 receivers free", 8, False, 15.7),
              ("4 receivers altitude", 4, True, 15.7))
TRUTH_EMITTERS = 400


def truth_list(oracle, name):
    """-> (receivers, the list, cfg keywords, true ECEF positions, the issue's error figure)"""
    _, n_rcv, alt, err = [r for r in TRUTH_ROWS if r[0] == name][0]
    rcv = receivers(n_rcv, seed=100 + n_rcv)
    pos, frames = emitters(oracle, TRUTH_EMITTERS, seed=200 + n_rcv)
    return rcv, build(rcv, pos, frames), dict(seconds_per_tick=SPT_NS, use_altitude=alt), pos, err


def case_lists(oracle):
    """The lists mirror, model and device are compared on: (name, receivers, list, cfg keywords).  Small: the model
    is a Python loop."""
    out = []
    for n_rcv, alt, n_em in ((6, False, 40), (8, False, 40), (4, True, 40), (4, False, 24), (3, True, 24), (5, False, 24),
                             (16, False, 12), (17, True, 12), (33, False, 6)):
        rcv = receivers(n_rcv, seed=300 + n_rcv)
        pos, frames = emitters(oracle, n_em, seed=400 + n_rcv + (50 if alt else 0))
        out.append((f"{n_rcv} receivers {'altitude' if alt else 'free'}", rcv, build(rcv, pos, frames),
                    dict(seconds_per_tick=SPT_NS, use_altitude=alt)))
    # 12 MHz ticks through rx[], with clock offsets, and some receivers missing per message
    rng = np.random.default_rng(7)
    rcv = receivers(9, seed=309, clock_offsets=rng.uniform(-1e-3, 1e-3, 9))
    pos, frames = emitters(oracle, 40, seed=409)
    heard = [sorted(rng.choice(9, size=int(rng.integers(2, 10)), replace=False).tolist()) for _ in pos]
    lst = build(rcv, pos, frames, spt=1 / 12e6, heard=heard, tick_base=5_000_000_000)
    out.append(("12 MHz ticks, offsets, partial", rcv, lst, dict(time_source=M.TIME_TICKS, use_altitude=True)))
    # the same receiver twice in some messages
    rcv = receivers(7, seed=307)
    pos, frames = emitters(oracle, 20, seed=407)
    lst = build(rcv, pos, frames, extra=[(i, i % 7, 40 + i) for i in range(0, 20, 2)])
    out.append(("repeated receivers", rcv, lst, dict(seconds_per_tick=SPT_NS)))
    return out


def many_receivers(oracle, n_rcv, n_em=2, seed=0):
    """n_rcv receivers (up to 256) on the rings, all hearing n_em emitters."""
    rcv = receivers(n_rcv, seed=500 + n_rcv + seed)
    pos, frames = emitters(oracle, n_em, seed=600 + n_rcv + seed)
    return rcv, build(rcv, pos, frames), dict(seconds_per_tick=SPT_NS)
