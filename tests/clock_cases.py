"""Scenarios for the clock-sync tests, built on tests/mlat_cases.py's receivers, emitters and build: every emitter's
frame is re-encoded to carry its own position (17-bit CPR, 25 ft), every receiver's clock gets an offset and a drift,
and the messages are spread over a span.  One message at a time goes through mlat_cases.build -- with the receivers'
clock offsets of that moment, offset + drift x t -- and the single-message lists are merged into one correlate result
with a receiver-major frame list beside it."""
import math

import numpy as np

from tests import fix_cases as FC
from tests import fix_model as F
from tests import mlat_cases as K
from tests import mlat_model as M
from tests import traffic

SPT_12MHZ = 1.0 / 12e6


def position_frames(oracle, pos, tc=11, displaced=None, altitude_code=None):
    """DF17 frames that say where the ECEF points `pos` are: CPR of the geodetic position, the nearest 25 ft altitude.
    displaced: {index: degrees added to the latitude before encoding} (a message that lies about its position)."""
    out = []
    for i, p in enumerate(pos):
        h, _, phi, lam = M.geodetic_of(p)
        lat, lon = math.degrees(phi) + (displaced or {}).get(i, 0.0), math.degrees(lam)
        yz, xz = F.cpr_encode(lat, lon, i & 1, False)
        code = K.altitude_code(h)[0] if altitude_code is None else altitude_code
        out.append(traffic.position_frame(oracle, 0x400000 + i, i & 1, yz, xz, alt_code=code, tc=tc))
    return out


def merge(parts, n_rcv):
    """Single-message lists of mlat_cases.build, in time order -> one list: msgs, recs, and the receiver-major frames /
    rx / counts with recs[].frame pointing into them."""
    recs = np.concatenate([p["recs"] for p in parts]) if parts else np.zeros(0, dtype=M.RECEPTION_DTYPE)
    msgs = np.concatenate([p["msgs"] for p in parts]) if parts else np.zeros(0, dtype=M.MESSAGE_DTYPE)
    frames = np.concatenate([p["frames"][p["recs"]["frame"]] for p in parts]) if parts else np.zeros(0, dtype=K.FRAME_DTYPE)
    rx = np.concatenate([p["rx"][p["recs"]["frame"]] for p in parts]) if parts else np.zeros(0, dtype=M.WIRE_RX_DTYPE)
    at = 0
    for g, p in enumerate(parts):
        msgs["first"][g] = at
        at += len(p["recs"])
    order = np.lexsort((np.arange(len(recs)), frames["offset"], recs["receiver"]))    # receiver-major, ascending T
    place = np.empty(len(recs), dtype=np.int64)
    place[order] = np.arange(len(recs))
    recs["frame"] = place
    counts = np.bincount(recs["receiver"], minlength=n_rcv).astype(np.uint64)
    return {"msgs": msgs, "recs": recs, "rx": rx[order], "frames": frames[order], "counts": counts}


def scenario(oracle, n_rcv, n_msgs, seed, span_s=60.0, spt=SPT_12MHZ, p_heard=0.7, offset_s=1e-3, drift=50e-6,
             heard=None, times=None, frames_of=None, tick_base=5_000_000_000, mod48=False, priors=None, extra=None,
             centre=(K.LAT0, K.LON0)):
    """n_msgs position messages over span_s seconds, each heard by every receiver with probability p_heard (heard: the
    receivers per message instead), by clocks offset_s and drift (bounds of uniform draws, or arrays) off.
    -> dict(rcv (clock_offset_s = the priors), lst, pos, offsets, drifts, t (emission times), cfg (time keywords))"""
    rng = np.random.default_rng(seed)
    offsets = rng.uniform(-offset_s, offset_s, n_rcv) if np.isscalar(offset_s) else np.asarray(offset_s, dtype=float)
    drifts = rng.uniform(-drift, drift, n_rcv) if np.isscalar(drift) else np.asarray(drift, dtype=float)
    rcv = K.receivers(n_rcv, seed=1000 + seed, centre=centre)
    pos, _ = K.emitters(oracle, n_msgs, seed=2000 + seed, centre=centre)
    frames = (frames_of or position_frames)(oracle, pos)
    t = np.sort(rng.uniform(0.5, span_s, n_msgs)) if times is None else np.asarray(times, dtype=float)
    if heard is None:
        heard = [[r for r in range(n_rcv) if rng.uniform() < p_heard] for _ in range(n_msgs)]
        heard = [h or [int(rng.integers(0, n_rcv))] for h in heard]               # every message is heard by someone
    parts = []
    for i in range(n_msgs):
        now = rcv.copy()
        now["clock_offset_s"] = offsets + drifts * t[i]
        parts.append(K.build(now, pos[i:i + 1], frames[i:i + 1], spt=spt, heard=[heard[i]], tick_base=tick_base,
                             spacing_s=float(t[i]), mod48=mod48,
                             extra=[(0, r, later) for (g, r, later) in (extra or ()) if g == i]))
    lst = merge(parts, n_rcv)
    if priors is not None:
        rcv["clock_offset_s"] = priors
    cfg = dict(time_source="ticks", seconds_per_tick=0.0 if spt == SPT_12MHZ else spt, seconds_per_time=spt)
    return {"rcv": rcv, "lst": lst, "pos": pos, "offsets": offsets, "drifts": drifts, "t": t, "cfg": cfg, "spt": spt,
            "heard": heard}


def truth(sc, reference=0):
    """(a, b) the scenario's clocks against the reference's, beyond the priors: the offsets at the first message's time."""
    if len(sc["lst"]["msgs"]) == 0:
        return np.zeros(len(sc["rcv"])), np.zeros(len(sc["rcv"]))
    t0 = sc["t"][0]
    now = sc["offsets"] + sc["drifts"] * t0
    a = (now - now[reference]) - (sc["rcv"]["clock_offset_s"] - sc["rcv"]["clock_offset_s"][reference])
    return a, sc["drifts"] - sc["drifts"][reference]


def case_lists(oracle):
    """The lists mirror, model and device are compared on: (name, scenario, sync keywords beyond the times)."""
    out = [("6 receivers, 12 MHz", scenario(oracle, 6, 120, seed=1), {}),
           ("8 receivers, 2 MHz", scenario(oracle, 8, 120, seed=2, spt=0.5e-6), {}),
           ("9 receivers, partial", scenario(oracle, 9, 100, seed=3, p_heard=0.4), dict(reference=4)),
           ("33 receivers, sparse", scenario(oracle, 33, 150, seed=4, p_heard=0.3, span_s=20.0), dict(min_rows=2)),
           ("2 receivers", scenario(oracle, 2, 30, seed=5, p_heard=1.0), {}),
           ("offsets only", scenario(oracle, 5, 60, seed=6, drift=0.0), dict(drift=False))]
    rng = np.random.default_rng(7)
    sc = scenario(oracle, 6, 80, seed=7, priors=None)
    sc["rcv"]["clock_offset_s"] = sc["offsets"] + rng.uniform(-2e-5, 2e-5, 6)        # coarse priors
    out.append(("coarse priors", sc, {}))
    # 510 unknowns from 510 rows: the worst conditioned list of the tests, so that the measured gaps cover it
    out.append(("256 receivers, two emitters", many_receivers(oracle), {}))
    return out


def many_receivers(oracle):
    """256 receivers, all hearing two emitters half a minute apart."""
    return scenario(oracle, 256, 2, seed=68, p_heard=1.0, times=[1.0, 31.0])


POLAR_CENTRE = (86.8, 179.8)


def polar(oracle):
    """6 receivers and 120 messages around (86.8, 179.8): the receivers lie on both sides of the antimeridian, the
    emitters on both sides of it and of the 87-degree latitude at which the zone count drops from 2 to 1."""
    return scenario(oracle, 6, 120, seed=12, centre=POLAR_CENTRE)


def exact_counts(sc, max_range_nm=180.0):
    """(n_eligible, n_rows) that the exact reference of tests/fix_cases.py predicts for a scenario's list: a message
    heard by two receivers or more, with an altitude, whose position the first reception's receiver accepts (no
    message of a scenario may be a tie); one row per further receiver."""
    lst, eligible, rows = sc["lst"], 0, 0
    for m in lst["msgs"]:
        mine = lst["recs"][int(m["first"]):int(m["first"]) + int(m["n_receptions"])]
        used = len(set(int(r) for r in mine["receiver"]))
        if used < 2 or M.altitude_of(m["bytes"]) is None:
            continue
        first = sc["rcv"][int(mine["receiver"][0])]
        d = FC.exact_decode((float(first["latitude"]), float(first["longitude"]), max_range_nm), bytes(m["bytes"]))
        assert not d["tie"]
        if d["verdict"] == FC.ACCEPTED and d["flags"] & (F.SURFACE | F.ALT) == F.ALT:
            eligible += 1
            rows += used - 1
    return eligible, rows


def outliers(oracle, seed=11, n_msgs=300, share=0.05):
    """The issue's outlier list: `share` of the messages displaced by 0.05 degrees.  -> (scenario, planted message set)"""
    rng = np.random.default_rng(seed)
    planted = set(int(i) for i in np.flatnonzero(rng.uniform(size=n_msgs) < share))
    sc = scenario(oracle, 6, n_msgs, seed=seed,
                  frames_of=lambda o, pos: position_frames(o, pos, displaced={i: 0.05 for i in planted}))
    return sc, planted
