"""Independent model of a track table's Comm-B side (include/adsb_hip.h, "Comm-B registers per aircraft"), written from
the header text in plain Python: a dict per aircraft and a sequential loop over the frames.  It has its own integer read
of an airborne-velocity message (DF17/18, type code 19, subtype 1-4) and Python's unbounded integers for every check.
Calls no library entry point; the registers' values come from tests/commb_model.py, the model of the stateless stage.
Shared by the CPU and GPU tiers."""
import math

import numpy as np

from tests import commb_model as CM

NOT_COMMB, EMPTY, NONE, ONE, AMBIGUOUS, SETTLED = range(6)
C50, C60 = CM.BIT[0x50], CM.BIT[0x60]
SELF, KNOWN, UNKNOWN, PARITY, UNSUPPORTED = range(5)          # adsb_modes_rec.kind
SPEED, DIRECTION, VRATE = 0x1, 0x2, 0x4                       # adsb_velocity.flags
UNTRACKED, UNADDRESSED = 0x2, 0x4
U32 = 2 ** 32 - 1
DEFAULT_CFG = dict(max_age_s=10.0, max_speed_diff_kt=40, max_vrate_diff_fpm=1000)

BLOCK_DTYPE = np.dtype([("time", "<f8"), ("value", "<i4", (5,)), ("status", "<u2"), ("settled", "<u2")])
MODEL_DTYPE = np.dtype([("bds40", BLOCK_DTYPE), ("bds50", BLOCK_DTYPE), ("bds60", BLOCK_DTYPE), ("n_commb", "<u4"),
                        ("n_settled", "<u4"), ("n_ambiguous", "<u4"), ("n_none", "<u4"), ("capability", "<u4"),
                        ("ra_word", "<u4"), ("ra_time", "<f8")])
OFFSETS = {"bds40": 0, "bds50": 32, "bds60": 64, "n_commb": 96, "n_settled": 100, "n_ambiguous": 104, "n_none": 108,
           "capability": 112, "ra_word": 116, "ra_time": 120}
assert MODEL_DTYPE.itemsize == 128 and BLOCK_DTYPE.itemsize == 32
assert all(MODEL_DTYPE.fields[k][1] == v for k, v in OFFSETS.items())
COUNTS = ("n_commb", "n_settled", "n_ambiguous", "n_none")
BLOCKS = {0x40: "bds40", 0x50: "bds50", 0x60: "bds60"}


# ---- the reference ---------------------------------------------------------------------------------------------------
def velocity_of(frame_bytes, time):
    """The exact fields of an airborne-velocity message as a dict, or None: type code 19, subtype 1-4.  ME bit 0 is the
    top bit of frame byte 4.  The caller decides that the frame is an accepted DF17/18."""
    b = bytes(frame_bytes)
    me = int.from_bytes(b[4:11], "big")
    f = lambda first, width: (me >> (56 - first - width)) & ((1 << width) - 1)
    st = f(5, 3)
    if f(0, 5) != 19 or not 1 <= st <= 4:
        return None
    k = 4 if st in (2, 4) else 1
    v = dict(time=time, subtype=st, flags=0, ew=0, ns=0, vr=0, airspeed=0, h10=0, tas=0)
    if st <= 2:
        if f(14, 10) != 0 and f(25, 10) != 0:
            v["ew"] = (-1 if f(13, 1) else 1) * (f(14, 10) - 1) * k
            v["ns"] = (-1 if f(24, 1) else 1) * (f(25, 10) - 1) * k
            v["flags"] |= SPEED | (DIRECTION if v["ew"] or v["ns"] else 0)       # as adsb_velocity; not read for ST 1-2
    else:
        if f(13, 1):
            v["h10"] = f(14, 10)
            v["flags"] |= DIRECTION
        if f(25, 10) != 0:
            v["airspeed"], v["tas"] = (f(25, 10) - 1) * k, f(24, 1)
            v["flags"] |= SPEED
    if f(37, 9) != 0:
        v["vr"] = (-1 if f(36, 1) else 1) * (f(37, 9) - 1) * 64
        v["flags"] |= VRATE
    return v


def velocity_of_record(rec):
    """The same dict from an adsb_velocity record (VELOCITY_DTYPE), reading only its exact fields; None if it holds no
    message."""
    st = int(rec["subtype"])
    if not 1 <= st <= 4:
        return None
    v = dict(time=float(rec["time"]), subtype=st, flags=int(rec["flags"]), ew=0, ns=0, vr=int(rec["vertical_rate_fpm"]),
             airspeed=0, h10=0, tas=0)
    if st <= 2:
        v["ew"], v["ns"] = int(rec["v_ew_kt"]), int(rec["v_ns_kt"])
    else:
        v["airspeed"], v["tas"] = int(rec["speed_kt"]), int(rec["airspeed_tas"])
        h = float(rec["direction_deg"]) * 128 / 45
        assert h == int(h)
        v["h10"] = int(h)
    return v


def usable(v, t_frame, max_age_s):
    if v is None:
        return False
    age = t_frame - v["time"]
    return 0 <= age <= max_age_s                                      # NaN: False


def sector16(ew, ns):
    a, b = abs(ew), abs(ns)
    if 985 * a < 408 * b:
        k = 0
    elif a < b:
        k = 1
    elif 408 * a < 985 * b:
        k = 2
    else:
        k = 3
    if ew >= 0 and ns > 0:
        return k
    if ew > 0 and ns <= 0:
        return 7 - k
    if ew <= 0 and ns < 0:
        return 8 + k
    return 15 - k


def circular(x, y, modulus):
    d = (x - y) % modulus
    return min(d, modulus - d)


def checks_50(status, value, v, cfg):
    """-> [True / False per check that applies]"""
    S, out = cfg["max_speed_diff_kt"], []
    ground = v["subtype"] <= 2 and v["flags"] & SPEED
    s2 = v["ew"] ** 2 + v["ns"] ** 2
    if status & 4 and ground:
        g = value[2]
        out.append(max(g - S, 0) ** 2 <= s2 <= (g + S) ** 2)
    if status & 2 and ground and s2 > 0:
        out.append(circular(value[1] >> 7, sector16(v["ew"], v["ns"]), 16) <= 1)
    if status & 16 and v["subtype"] >= 3 and v["flags"] & SPEED and v["tas"] == 1:
        out.append(abs(value[4] - v["airspeed"]) <= S)
    return out


def checks_60(status, value, v, cfg):
    S, V, out = cfg["max_speed_diff_kt"], cfg["max_vrate_diff_fpm"], []
    ground = v["subtype"] <= 2 and v["flags"] & SPEED
    s2 = v["ew"] ** 2 + v["ns"] ** 2
    if status & 1 and ground and s2 > 0:
        out.append(circular(value[0] >> 7, sector16(v["ew"], v["ns"]), 16) <= 2)
    if status & 1 and v["subtype"] >= 3 and v["flags"] & DIRECTION:
        out.append(circular(value[0], 2 * v["h10"], 2048) <= 128)
    if status & 2 and v["subtype"] >= 3 and v["flags"] & SPEED and v["tas"] == 0:
        out.append(abs(value[1] - v["airspeed"]) <= S)
    if status & 8 and v["flags"] & VRATE:
        out.append(abs(value[3] - v["vr"]) <= V)
    if status & 16 and v["flags"] & VRATE:
        out.append(abs(value[4] - v["vr"]) <= V)
    return out


def decide(frame_bytes, v, cfg):
    """-> 0x50, 0x60 or None for the MB of this frame against a USABLE reference"""
    m = CM.MB(bytes(frame_bytes)[4:11])
    s5, v5, _ = CM.values(m, 0x50)
    s6, v6, _ = CM.values(m, 0x60)
    c5, c6 = checks_50(s5, v5, v, cfg), checks_60(s6, v6, v, cfg)
    supported = lambda c: len(c) > 0 and all(c)
    contradicted = lambda c: not all(c)
    if supported(c5) and contradicted(c6):
        return 0x50
    if supported(c6) and contradicted(c5):
        return 0x60
    return None


def settle(frame_bytes, rec, v, t_frame, cfg=DEFAULT_CFG):
    """The per-frame output of a COUNTED frame: rec (a REC_DTYPE record) itself, or the settled record."""
    out = np.array(rec, dtype=CM.REC_DTYPE)
    if int(rec["state"]) != AMBIGUOUS or int(rec["candidates"]) != C50 | C60 or not usable(v, t_frame, cfg["max_age_s"]):
        return out
    bds = decide(frame_bytes, v, cfg)
    if bds is None:
        return out
    status, value, word = CM.values(CM.MB(bytes(frame_bytes)[4:11]), bds)
    out["state"], out["bds"], out["status"], out["value"], out["word"] = SETTLED, bds, status, value, word
    return out


# ---- the side record -------------------------------------------------------------------------------------------------
def empty_block():
    return dict(time=math.nan, value=[0] * 5, status=0, settled=0)


def empty():
    return dict(bds40=empty_block(), bds50=empty_block(), bds60=empty_block(), n_commb=0, n_settled=0, n_ambiguous=0,
                n_none=0, capability=0, ra_word=0, ra_time=math.nan)


def record(d):
    out = np.zeros(1, dtype=MODEL_DTYPE)
    for k, v in d.items():
        if k in BLOCKS.values():
            for kk, vv in v.items():
                out[k][kk][0] = vv
        else:
            out[k][0] = v
    return out[0]


def as_dict(rec):
    d = {}
    for k in MODEL_DTYPE.names:
        if k in BLOCKS.values():
            d[k] = dict(time=float(rec[k]["time"]), value=[int(x) for x in rec[k]["value"]], status=int(rec[k]["status"]),
                        settled=int(rec[k]["settled"]))
        else:
            d[k] = rec[k].item()
    return d


def count(a, out, time):
    """One COUNTED frame's per-frame output applied to the aircraft's dict `a`, in place."""
    state, bds = int(out["state"]), int(out["bds"])
    assert state != NOT_COMMB
    a["n_commb"] = min(a["n_commb"] + 1, U32)
    if state == NONE:
        a["n_none"] = min(a["n_none"] + 1, U32)
    if state == AMBIGUOUS:
        a["n_ambiguous"] = min(a["n_ambiguous"] + 1, U32)
    if state == SETTLED:
        a["n_settled"] = min(a["n_settled"] + 1, U32)
    if state in (ONE, SETTLED) and bds in BLOCKS:
        a[BLOCKS[bds]] = dict(time=time, value=[int(x) for x in out["value"]], status=int(out["status"]),
                              settled=1 if state == SETTLED else 0)
    if state == ONE and bds == 0x17 and int(out["word"]) != 0:
        a["capability"] = int(out["word"])
    if state == ONE and bds == 0x30:
        a["ra_word"], a["ra_time"] = int(out["word"]), time
    return a


def merge(into, later):
    """`into` followed by `later` (dicts), by the header's combine -> a new dict"""
    o = {k: (dict(v) if isinstance(v, dict) else v) for k, v in into.items()}
    for b in BLOCKS.values():
        if not math.isnan(later[b]["time"]):
            o[b] = dict(later[b])
    if later["capability"]:
        o["capability"] = later["capability"]
    if not math.isnan(later["ra_time"]):
        o["ra_word"], o["ra_time"] = later["ra_word"], later["ra_time"]
    for k in COUNTS:
        o[k] = min(into[k] + later[k], U32)
    return o


class Table:
    """The table as the header defines it: {address: dict(commb = side-record dict, vel = the newest airborne-velocity
    message or None)}, admitted in ascending address per update while there is room."""

    def __init__(self, max_aircraft=65536, seconds_per_sample=0.5e-6, cfg=None, reserved=True):
        self.state, self.cap, self.sps = {}, max_aircraft, seconds_per_sample
        self.cfg = dict(DEFAULT_CFG, **(cfg or {}))
        self.reserved = reserved

    def reserve(self):
        """aircraft held from before the reserve have the EMPTY record"""
        self.reserved = True

    def update(self, frames, recs, commb=None, sample_base=0):
        """update_commb (commb given) or update_modes (None: only admission and the held velocity move).
        -> frame_commb (REC_DTYPE), or None"""
        n = len(frames)
        ok = [int(recs[j]["kind"]) in (SELF, KNOWN) for j in range(n)]
        addr = [int(recs[j]["address"]) & 0xFFFFFF for j in range(n)]
        new = sorted({addr[j] for j in range(n) if ok[j]} - set(self.state))
        for a in new[:self.cap - len(self.state)]:
            self.state[a] = dict(commb=empty(), vel=None)
        out = None if commb is None else np.array(commb, dtype=CM.REC_DTYPE)
        for j in range(n):
            if not ok[j] or addr[j] not in self.state:
                continue
            a, b = self.state[addr[j]], frames["bytes"][j].tobytes()
            t = float(sample_base + int(frames["offset"][j])) * self.sps
            if commb is not None and int(commb[j]["state"]) != NOT_COMMB:                 # counted
                out[j] = settle(b, commb[j], a["vel"], t, self.cfg)
                count(a["commb"], out[j], t)
            if int(recs[j]["df"]) in (17, 18):
                v = velocity_of(b, t)
                if v is not None:
                    a["vel"] = v
        return out

    def expire(self, addresses):
        for a in addresses:
            del self.state[a]

    def reset(self):
        self.state = {}

    def records(self):
        """The side records in ascending address, as fetch_commb returns them"""
        out = np.zeros(len(self.state), dtype=MODEL_DTYPE)
        for k, a in enumerate(sorted(self.state)):
            out[k] = record(self.state[a]["commb"])
        return out


def same_records(got, want, what=""):
    got = np.ascontiguousarray(got)
    assert got.dtype.itemsize == 128 and len(got) == len(want), (what, len(got), len(want))
    if got.tobytes() != want.tobytes():
        g = got.view(MODEL_DTYPE)
        bad = [k for k in range(len(want)) if g[k].tobytes() != want[k].tobytes()][:4]
        raise AssertionError((what, [(k, g[k], want[k]) for k in bad]))


def same_frames(got, want, what=""):
    got = np.ascontiguousarray(got)
    assert got.dtype.itemsize == 32 and len(got) == len(want), (what, len(got), len(want))
    if got.tobytes() != want.tobytes():
        g = got.view(CM.REC_DTYPE)
        bad = [k for k in range(len(want)) if g[k].tobytes() != want[k].tobytes()][:4]
        raise AssertionError((what, [(k, g[k], want[k]) for k in bad]))
