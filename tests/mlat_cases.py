"""Scenarios for the multilaterate tests: receivers on rings around (47.45, 8.56), emitters out to 150 km, every message
a real DF17 airborne-position frame, reception ticks from exact ECEF distances -- built straight into a correlate
result (MESSAGE_DTYPE, RECEPTION_DTYPE, with the WIRE_RX_DTYPE records of TIME_TICKS beside it), and the small
hand-made lists of the edge tests: edge_lists, every outcome and cfg field of the solver on 8 to 16 messages each, with
the literal expectations check_expectations holds a result to."""
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
        rx[j] = (rows[k][2] % (1 << 48 if mod48 else 1 << 64), 0, 0, ord("3"), rows[k][1])
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


# ---- the edge lists: every outcome and every cfg field, small enough for the model, with literal expectations ----

def edge_frame(first_byte, tc, code, icao=0x4C0000):
    """A 112-bit frame with the given first byte (DF << 3 | CA), type code and 12-bit altitude code, zero CPR fields and
    NO valid CRC: multilaterate reads bytes 0, 4, 5 and 6 and never the parity."""
    return bytes([first_byte, icao >> 16 & 0xFF, icao >> 8 & 0xFF, icao & 0xFF, tc << 3, code >> 4 & 0xFF,
                  (code & 0xF) << 4]) + bytes(7)


def q_code(n):
    """The 12-bit altitude code with the Q bit of n x 25 ft - 1000 ft, n < 2048."""
    return (n >> 4) << 5 | 0x10 | (n & 0xF)


FT = 0.3048
# item 7, one message per row: (what, first byte, type code, altitude code, the height it decodes to or None)
ALTITUDE_ROWS = (("TC 8", 0x8D, 8, q_code(1352), None), ("TC 9", 0x8D, 9, q_code(1352), 32800 * FT),
                 ("TC 18", 0x8D, 18, q_code(1352), 32800 * FT), ("TC 19", 0x8D, 19, q_code(1352), None),
                 ("DF18 TC 11", 0x90, 11, q_code(700), 16500 * FT), ("DF20 as TC 11", 0xA0, 11, q_code(700), None),
                 ("DF11 as TC 11", 0x58, 11, q_code(700), None), ("code 0", 0x8D, 11, 0, None),
                 ("Gillham, Q clear", 0x8D, 11, 0x3A8, None), ("smallest Q code", 0x8D, 11, q_code(0), -1000 * FT),
                 ("largest Q code", 0x8D, 11, q_code(2047), 50175 * FT))
assert q_code(0) == 0x010 and q_code(2047) == 0xFFF and not 0x3A8 & 0x10

# item 8: (centre, whether its receivers must lie on both sides of the antimeridian)
GLOBE_CENTRES = (((86.8, 179.8), True), ((-86.8, -179.8), True), ((0.0, 179.95), True), ((0.01, -0.01), False),
                 ((-33.9, 18.4), False))


def placed(heights, seed, max_range=150e3, centre=(LAT0, LON0)):
    """ECEF positions at the given heights, 0-max_range out from `centre` (the emitters of frames made by hand)."""
    rng = np.random.default_rng(seed)
    pos = []
    for h in heights:
        az, rad = rng.uniform(0, 2 * math.pi), max_range * math.sqrt(rng.uniform(0, 1))
        pos.append(M.ecef_of(*_offset(centre[0], centre[1], rad * math.sin(az), rad * math.cos(az)), h))
    return np.array(pos)


def idents(oracle, n, base=0x4B0000):
    return [traffic.ident_frame(oracle, base + i, [1 + (i + k) % 26 for k in range(8)]) for i in range(n)]


def _centroid_distance(rcv, fix):
    st = np.array([M.ecef_of(r["latitude"], r["longitude"], r["height_m"]) for r in rcv])
    return float(np.sqrt(((M.ecef_of(fix["latitude"], fix["longitude"], fix["height_m"]) - st.mean(axis=0)) ** 2).sum()))


def _between_4th_and_5th(values):
    """The geometric mean of the 4th and 5th smallest value, which must lie at least 1 % apart: no rounding moves a
    fix across.  -> (the threshold, the indices above it)"""
    order = np.argsort(values)
    lo, hi = float(values[order[3]]), float(values[order[4]])
    assert lo > 0 and hi >= 1.01 * lo, (lo, hi)
    return math.sqrt(lo * hi), sorted(int(k) for k in order[4:])


def edge_lists(oracle):
    """-> [(name, receivers, list, cfg keywords, expect)], 6 receivers and 8 emitters unless the item says otherwise.
    expect: what check_expectations holds a result of that list to (the keys are explained there); lists that are
    compared with each other name each other."""
    NS = dict(seconds_per_tick=SPT_NS)
    out = []
    rcv6 = receivers(6, seed=1106)
    pos8, frames8 = emitters(oracle, 8, seed=1208)
    plain = build(rcv6, pos8, frames8)

    # 1. all five stations equal: SINGULAR, free and with altitude
    same = receivers(5, seed=1105)
    same[:] = same[0]
    lst = build(same, pos8, frames8)
    for alt in (False, True):
        out.append((f"singular {'altitude' if alt else 'free'}", same, lst, dict(NS, use_altitude=alt),
                    dict(all_set=M.ATTEMPTED | M.SINGULAR, none_set=M.VALID, n_valid=0, n_used=[5] * 8)))

    # 2a. the 48-bit tick wrap
    a = build(rcv6, pos8, frames8, spt=1 / 12e6, tick_base=1000)
    b = build(rcv6, pos8, frames8, spt=1 / 12e6, tick_base=(1 << 48) - 100_000, mod48=True)
    assert 0 < (b["rx"]["ticks"] < (1 << 47)).sum() < len(b["rx"])                  # the list straddles 2^48
    ticks = dict(time_source=M.TIME_TICKS)
    out.append(("ticks from 1000", rcv6, a, ticks, dict(all_set=M.VALID)))
    out.append(("ticks across 2^48", rcv6, b, ticks, dict(all_set=M.VALID, same_bytes_as="ticks from 1000")))
    # 2b. reception times at 1 ns from 12345, from 2^63 + 12345 and across 2^64
    for base, name in ((12345, "times from 12345"), ((1 << 63) + 12345, "times from 2^63"),
                       ((1 << 64) - 3_000_000, "times across 2^64")):
        lst = build(rcv6, pos8, frames8, tick_base=base)
        if base > (1 << 63) + 12345:
            early = lst["recs"]["time"] < (1 << 63)
            assert 0 < early.sum() < len(early)                                     # times on both sides of the wrap
        elif base > 12345:
            assert (lst["recs"]["time"] >= (1 << 63)).all()
        out.append((name, rcv6, lst, NS, dict(all_set=M.VALID, **({} if base == 12345 else
                                                                   {"same_bytes_as": "times from 12345"}))))
    # 2c. declared clock offsets of +-1 ms, exact in ticks
    out.append(("plain", rcv6, plain, NS, dict(all_set=M.VALID)))
    off_ticks = np.array([1, -1, 1, -1, 1, -1]) * 1_000_000
    declared = rcv6.copy()
    declared["clock_offset_s"] = off_ticks * SPT_NS
    out.append(("declared offsets", declared, build(rcv6, pos8, frames8, offset_ticks=off_ticks), NS,
                dict(all_set=M.VALID, same_position_as="plain")))

    # 3. rejections between neighbours: the thresholds from the model's unrejected run
    free, _, _ = M.multilaterate(rcv6, plain["msgs"], plain["recs"], **NS)
    assert (free["flags"] & M.VALID != 0).all()
    limit, over = _between_4th_and_5th(free["residual_rms_m"].astype(np.float64))
    out.append(("residual limit", rcv6, plain, dict(NS, max_residual_m=limit),
                dict(rejected=(M.REJECTED_RESIDUAL, over, "plain"), n_valid=4)))
    limit, over = _between_4th_and_5th(np.array([_centroid_distance(rcv6, f) for f in free]))
    out.append(("range limit", rcv6, plain, dict(NS, max_range_m=limit),
                dict(rejected=(M.REJECTED_RANGE, over, "plain"), n_valid=4)))

    # 4. min_receivers = 5 with altitude: 3, 4, 5, 6, 3, 4, 5, 6 receivers hear the message
    n_heard = [3, 4, 5, 6, 3, 4, 5, 6]
    lst = build(rcv6, pos8, frames8, heard=[list(range(n)) for n in n_heard])
    few = [n < 5 for n in n_heard]
    out.append(("min_receivers 5", rcv6, lst, dict(NS, use_altitude=True, min_receivers=5),
                dict(exactly={M.TOO_FEW: few, M.ATTEMPTED: [not f for f in few]}, n_used=n_heard,
                     zero_position=[k for k in range(8) if few[k]])))

    # 5. iteration caps and step tolerances: position frames (one stage) alternate with identification frames (two)
    # the first four emitters within 3 km of the centre, where three steps reach a 1 m step and not a 0.1 mm one
    near, near_frames = emitters(oracle, 4, seed=1209, max_range=3e3)
    pos = np.concatenate([near, pos8[4:]])
    mixed = [f if k % 2 == 0 else g for k, (f, g) in enumerate(zip(near_frames + frames8[4:], idents(oracle, 8)))]
    lst = build(rcv6, pos, mixed)
    stages = [1 + k % 2 for k in range(8)]
    for cap in (1, 2, 3):
        for tol in (1.0, 1e-4):
            expect = dict(all_set=M.ATTEMPTED, cap=(cap, stages), has_position=True,
                          exactly={M.ALTITUDE: [k % 2 == 0 for k in range(8)]})
            if cap == 3 and tol == 1.0:
                expect["more_converged_than"] = "cap 3 tol 0.0001"
            out.append((f"cap {cap} tol {tol:g}", rcv6, lst,
                        dict(NS, use_altitude=True, max_iterations=cap, step_tol_m=tol), expect))
    out[-1], out[-2] = out[-2], out[-1]                      # the 0.1 mm run before the 1 m run that is compared with it

    # 6. default_altitude_m: identification frames, no altitude; the start differs, the fix does not
    lst = build(rcv6, pos8, idents(oracle, 8))
    out.append(("default altitude 10000", rcv6, lst, NS, dict(all_set=M.VALID, none_set=M.ALTITUDE)))
    out.append(("default altitude 3000", rcv6, lst, dict(NS, default_altitude_m=3000.0),
                dict(all_set=M.VALID, none_set=M.ALTITUDE, same_position_as="default altitude 10000",
                     other_iterations_than="default altitude 10000")))

    # 7. the altitude decode's edges, one message per row, the emitter at the height its code decodes to
    pos = placed([10000.0 if h is None else h for *_, h in ALTITUDE_ROWS], seed=1307)
    lst = build(rcv6, pos, [edge_frame(b0, tc, code, 0x4C0000 + k) for k, (_, b0, tc, code, _) in enumerate(ALTITUDE_ROWS)])
    has = [h is not None for *_, h in ALTITUDE_ROWS]
    out.append(("altitude decode", rcv6, lst, dict(NS, use_altitude=True),
                dict(all_set=M.ATTEMPTED, exactly={M.ALTITUDE: has}, valid_where=has)))

    # 8. where on the globe: near both poles across the antimeridian, on the equator at it, at (0, 0), in the south
    for k, ((lat, lon), straddles) in enumerate(GLOBE_CENTRES):
        rcv = receivers(6, seed=1400 + k, centre=(lat, lon))
        pos, frames = emitters(oracle, 8, seed=1500 + k, centre=(lat, lon))
        assert (np.abs(rcv["latitude"]) < 90.0).all()
        for p in pos:
            assert abs(math.degrees(M.geodetic_of(p)[2])) < 90.0
        if straddles:
            assert (rcv["longitude"] > 90.0).any() and (rcv["longitude"] < -90.0).any()
        for alt in (False, True):
            out.append((f"globe ({lat:g}, {lon:g}) {'altitude' if alt else 'free'}", rcv, build(rcv, pos, frames),
                        dict(NS, use_altitude=alt), dict(all_set=M.ATTEMPTED, min_valid=7, truth=pos)))

    # 10. one wavefront of everything: each group of four lanes holds a singular, a too-few, a capped and a converging one
    out.append(one_wavefront(oracle))
    return out


def one_wavefront(oracle):
    """16 messages under one cfg (use_altitude, min_receivers 4, max_iterations 3), message 4 q + r being of kind r:
    0 heard only by five equal stations (SINGULAR), 1 heard by three (TOO_FEW), 2 an identification frame far out (two
    stages of three steps: not converged), 3 an altitude-edge frame near the centre (converged inside three steps)."""
    rcv = np.concatenate([receivers(6, seed=1106), np.repeat(receivers(1, seed=1601), 5)])
    far, far_frames = emitters(oracle, 12, seed=1602)
    edge_rows = [r for r in ALTITUDE_ROWS if r[4] is not None][-4:]     # TC 18, DF18, the smallest and the largest code
    near = placed([r[4] for r in edge_rows], seed=1603, max_range=3e3)
    ident = idents(oracle, 4, base=0x4D0000)
    pos, frames, heard = [], [], []
    for q in range(4):
        pos += [far[3 * q], far[3 * q + 1], far[3 * q + 2], near[q]]
        frames += [far_frames[3 * q], far_frames[3 * q + 1], ident[q],
                   edge_frame(edge_rows[q][1], edge_rows[q][2], edge_rows[q][3], 0x4E0000 + q)]
        heard += [list(range(6, 11)), [q, (q + 2) % 6, (q + 4) % 6], list(range(6)), list(range(6))]
    kind = lambda r: [k % 4 == r for k in range(16)]
    cfg = dict(seconds_per_tick=SPT_NS, use_altitude=True, min_receivers=4, max_iterations=3)
    return ("one wavefront of everything", rcv, build(rcv, np.array(pos), frames, heard=heard), cfg,
            dict(exactly={M.SINGULAR: kind(0), M.TOO_FEW: kind(1), M.VALID: kind(3),
                          M.ATTEMPTED: [k % 4 != 1 for k in range(16)]},
                 flags_of={k: (M.TOO_FEW, M.ATTEMPTED, M.ATTEMPTED | M.ALTITUDE | M.CONVERGED | M.VALID)[k % 4 - 1]
                           for k in range(16) if k % 4},
                 n_used=[5, 3, 6, 6] * 4, cap=(3, [1, 0, 2, 1] * 4), one_at_a_time=True))


def check_expectations(name, fixes, hdr, expect, results, lasts=None, step_tol=0.01, model_error=None):
    """Holds one result (fixes and header of the list `name`) to its literal expectations.  results: {name: fixes} of
    the lists run before, by the same solver.  lasts: the model's last step lengths.  The keys:
      all_set / none_set       flag bits every fix has / no fix has
      exactly {flag: [bool]}   the flag is set exactly where the list says
      flags_of {k: flags}      the whole flag word of fix k
      more_converged_than name some fix is CONVERGED here and not in that list's result, none the other way round
      valid_where [bool]       VALID wherever the list says (elsewhere either)
      n_used [int], n_valid int, min_valid int (header and fixes)
      zero_position [k]        the 48 position bytes and iterations of fix k are zero
      has_position             every fix reports a non-zero position
      cap (cap, [stages])      iterations <= cap x stages; with cap 1, a fix whose model last step is >= the step tolerance
                               is neither CONVERGED nor VALID
      same_bytes_as name       byte-equal to that list's fixes
      same_position_as name    positions within the mirror-vs-model tolerance of that list's, the same flags
      other_iterations_than    at least one fix differs in iterations from that list's
      rejected (flag, [k], base name)   exactly the fixes k carry the flag and lose VALID against the base list, every
                               other bit and every position byte kept
      truth [ECEF]             longitudes in (-180, 180]; with model_error (the model's largest error on this list), every
                               VALID fix within 3 x model_error of its true position
    A SINGULAR fix has zero dilutions.  -> the largest error against the truth, or None."""
    flags = fixes["flags"].astype(np.int64)
    n = len(fixes)
    assert int(hdr["n_messages"]) == n and int(hdr["flags"]) == 0, name
    assert int(hdr["n_attempted"]) == int((flags & M.ATTEMPTED != 0).sum()), name
    assert int(hdr["n_valid"]) == int((flags & M.VALID != 0).sum()), name
    assert (fixes["reserved"] == 0).all(), name
    sing = flags & M.SINGULAR != 0
    assert (fixes["pdop"][sing] == 0).all() and (fixes["hdop"][sing] == 0).all() and (fixes["vdop"][sing] == 0).all(), name
    assert (flags[sing] & M.VALID == 0).all(), name
    if "all_set" in expect:
        assert (flags & expect["all_set"] == expect["all_set"]).all(), (name, flags)
    if "none_set" in expect:
        assert (flags & expect["none_set"] == 0).all(), (name, flags)
    for flag, where in expect.get("exactly", {}).items():
        assert (flags & flag != 0).tolist() == list(where), (name, hex(flag), flags)
    for k, literal in expect.get("flags_of", {}).items():
        assert flags[k] == literal, (name, k, flags)
    if "more_converged_than" in expect:
        other = results[expect["more_converged_than"]]["flags"]
        assert ((flags & M.CONVERGED != 0) & (other & M.CONVERGED == 0)).any() and (flags | other == flags).all(), name
    if "valid_where" in expect:
        assert (flags & M.VALID != 0)[np.array(expect["valid_where"])].all(), (name, flags)
    if "n_used" in expect:
        assert fixes["n_used"].tolist() == list(expect["n_used"]), name
    if "n_valid" in expect:
        assert int(hdr["n_valid"]) == expect["n_valid"], name
    if "min_valid" in expect:
        assert int(hdr["n_valid"]) >= expect["min_valid"], (name, flags)
    for k in expect.get("zero_position", ()):
        assert fixes[k].tobytes()[:48] == bytes(48) and fixes["iterations"][k] == 0, (name, k)
    if expect.get("has_position"):
        assert (fixes["latitude"] != 0).all() and (fixes["longitude"] != 0).all() and np.isfinite(fixes["height_m"]).all(), name
    if "cap" in expect:
        cap, stages = expect["cap"]
        assert (fixes["iterations"] <= cap * np.array(stages)).all(), (name, fixes["iterations"])
        if cap == 1 and lasts is not None:
            long_step = np.array([s > 0 and last >= step_tol for s, last in zip(stages, lasts)])
            assert long_step.any() and (flags[long_step] & (M.CONVERGED | M.VALID) == 0).all(), (name, flags, lasts)
    if "same_bytes_as" in expect:
        assert fixes.tobytes() == results[expect["same_bytes_as"]].tobytes(), name
    if "same_position_as" in expect:
        other = results[expect["same_position_as"]]
        assert (flags == other["flags"]).all(), name
        gap = max(M.position_gap_m(x, y) for x, y in zip(fixes, other))
        assert gap <= M.MIRROR_VS_MODEL_TOL_M, (name, gap)
    if "other_iterations_than" in expect:
        assert (fixes["iterations"] != results[expect["other_iterations_than"]]["iterations"]).any(), name
    if "rejected" in expect:
        flag, where, base = expect["rejected"]
        base = results[base]
        hit = np.zeros(n, dtype=bool)
        hit[where] = True
        assert hit.sum() == 4 and (base["flags"] & M.VALID != 0).all(), name
        assert (flags == np.where(hit, (base["flags"] ^ M.VALID) | flag, base["flags"])).all(), (name, flags)
        for f, g in zip(fixes, base):
            assert f.tobytes()[:52] == g.tobytes()[:52], name                 # a rejected fix still says where
    worst = None
    if "truth" in expect:
        valid = flags & M.VALID != 0
        assert ((fixes["longitude"][valid] > -180.0) & (fixes["longitude"][valid] <= 180.0)).all(), name
        assert (np.abs(fixes["latitude"][valid]) <= 90.0).all(), name
        worst = max(float(np.sqrt(((M.ecef_of(f["latitude"], f["longitude"], f["height_m"]) - p) ** 2).sum()))
                    for f, p in zip(fixes[valid], np.asarray(expect["truth"])[valid]))
        if model_error is not None:
            assert worst <= 3 * model_error, (name, worst, model_error)
    return worst


_MODELLED = []


def modelled(oracle):
    """[(name, receivers, list, cfg, expect or None, the model's fixes, its header, its last step lengths)] of the case
    lists and then the edge lists: the model runs once per session, and nobody writes to what it returned."""
    if not _MODELLED:
        both = [(n, r, l, c, None) for n, r, l, c in case_lists(oracle)] + edge_lists(oracle)
        for name, rcv, lst, cfg, expect in both:
            want, hdr, lasts = M.multilaterate(rcv, lst["msgs"], lst["recs"], lst["rx"], **cfg)
            for arr in (want, lasts):
                arr.setflags(write=False)
            _MODELLED.append((name, rcv, lst, cfg, expect, want, hdr, lasts))
    return _MODELLED
