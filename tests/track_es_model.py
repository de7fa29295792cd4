"""Independent sequential model of a track table's extended squitter step (include/adsb_hip.h, "Extended squitter status
per aircraft"), in plain Python: it walks the list frame by frame and keeps one dict per aircraft, so it has no scan, no
segments and no merge of parts.  The per-frame record is tests/es_model.py's; the integrity table is this file's own
copy, written as a table of rows, and every row a resolution uses is noted in Table.reached so that a case list can show
which rows it reaches.  Calls no library entry point.  Shared by the CPU and GPU tiers."""
import math

import numpy as np

from tests import es_model as M

COUNTED, POSITION, VERSIONED, STALE_A, STALE_C = 1, 2, 4, 8, 16
U32 = 0xFFFFFFFF
SELF, KNOWN = 0, 1                                       # adsb_modes_rec.kind of an accepted frame
BLOCKS = ("operational_airborne", "operational_surface", "target_state", "emergency", "acas_ra")
FRAME_ES_DTYPE = np.dtype([("rc_dm", "<u4"), ("nic", "u1"), ("version", "u1"), ("supp", "u1"), ("flags", "u1")])
MODEL_DTYPE = np.dtype([(k, M.REC_DTYPE) for k in BLOCKS] + [("time", "<f8", (5,))]
                       + [(k, "<f8") for k in ("version_time", "nic_a_time", "nic_c_time", "position_time")]
                       + [("rc_dm", "<u4")]
                       + [(k, "u1") for k in ("nic", "position_tc", "nic_b", "position_supp", "version", "nic_a", "nic_c", "category")]
                       + [("n_es", "<u4"), ("n_position", "<u4")] + [(k, "u1") for k in ("nac_v", "velocity_flags", "has", "reserved")])
assert MODEL_DTYPE.itemsize == 256 and FRAME_ES_DTYPE.itemsize == 8

# ---- the integrity table, row by row ---------------------------------------------------------------------------------
# (type codes, version column, supplements "ABC" with - for "any", NIC, Rc in metres as printed, "-" unknown).  Version
# column 0 is an aircraft of version 0 or of no known version: NIC 0 and the radius the type code alone gives.
ROWS = (
    ((0, 18, 22), 0, "---", 0, "-"), ((9, 20, 5), 0, "---", 0, "7.5"), ((10, 21, 6), 0, "---", 0, "25"),
    ((11, 7), 0, "---", 0, "185.2"), ((12,), 0, "---", 0, "370.4"), ((13,), 0, "---", 0, "926"), ((14,), 0, "---", 0, "1852"),
    ((15,), 0, "---", 0, "3704"), ((16,), 0, "---", 0, "18520"), ((17,), 0, "---", 0, "37040"), ((8,), 0, "---", 0, "-"),
    # version 1: supplement A only
    ((0, 18, 22), 1, "---", 0, "-"), ((9, 20, 5), 1, "---", 11, "7.5"), ((10, 21, 6), 1, "---", 10, "25"),
    ((11,), 1, "1--", 9, "75"), ((11,), 1, "0--", 8, "185.2"), ((12,), 1, "---", 7, "370.4"),
    ((13,), 1, "1--", 6, "1111.2"), ((13,), 1, "0--", 6, "926"), ((14,), 1, "---", 5, "1852"), ((15,), 1, "---", 4, "3704"),
    ((16,), 1, "1--", 3, "7408"), ((16,), 1, "0--", 2, "14816"), ((17,), 1, "---", 1, "37040"),
    ((7,), 1, "1--", 9, "75"), ((7,), 1, "0--", 8, "185.2"), ((8,), 1, "---", 0, "-"),
    # version 2 and above: A with B airborne, A with C on the surface
    ((0, 18, 22), 2, "---", 0, "-"), ((9, 20, 5), 2, "---", 11, "7.5"), ((10, 21, 6), 2, "---", 10, "25"),
    ((11,), 2, "11-", 9, "75"), ((11,), 2, "10-", 8, "185.2"), ((11,), 2, "0--", 8, "185.2"), ((12,), 2, "---", 7, "370.4"),
    ((13,), 2, "1--", 6, "1111.2"), ((13,), 2, "01-", 6, "555.6"), ((13,), 2, "00-", 6, "926"),
    ((14,), 2, "---", 5, "1852"), ((15,), 2, "---", 4, "3704"),
    ((16,), 2, "11-", 3, "7408"), ((16,), 2, "10-", 2, "14816"), ((16,), 2, "0--", 2, "14816"), ((17,), 2, "---", 1, "37040"),
    ((7,), 2, "1-0", 9, "75"), ((7,), 2, "1-1", 8, "185.2"), ((7,), 2, "0--", 8, "185.2"),
    ((8,), 2, "1-1", 7, "370.4"), ((8,), 2, "1-0", 6, "555.6"), ((8,), 2, "0-1", 6, "1111.2"), ((8,), 2, "0-0", 0, "-"),
)
DM = {"-": 0, "7.5": 75, "25": 250, "75": 750, "185.2": 1852, "370.4": 3704, "555.6": 5556, "926": 9260, "1111.2": 11112,
      "1852": 18520, "3704": 37040, "7408": 74080, "14816": 148160, "18520": 185200, "37040": 370400}


def integrity_row(tc, version, supp):
    """the index of the one row of ROWS that applies"""
    column = 0 if version == M.VERSION_UNKNOWN else min(version, 2)
    abc = f"{supp & 1}{supp >> 1 & 1}{supp >> 2 & 1}"
    hits = [k for k, (tcs, v, pattern, _, _) in enumerate(ROWS)
            if tc in tcs and v == column and all(p in ("-", s) for p, s in zip(pattern, abc))]
    assert len(hits) == 1, (tc, version, supp, hits)
    return hits[0]


def integrity(tc, version, supp):
    _, _, _, nic, rc = ROWS[integrity_row(tc, version, supp)]
    return nic, DM[rc]


def _rows_are_whole():
    """every position type code x version column x supplement set meets exactly one row, and the table says what
    tests/es_model.py's says"""
    for tc in (0, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 20, 21, 22):
        for version in (0, 1, 2, 5, M.VERSION_UNKNOWN):
            for supp in range(8):
                assert integrity(tc, version, supp) == M.integrity(tc, version, supp), (tc, version, supp)


_rows_are_whole()


# ---- the side record ---------------------------------------------------------------------------------------------------
def empty():
    d = dict(blocks=[None] * 5, time=[math.nan] * 5, version_time=math.nan, nic_a_time=math.nan, nic_c_time=math.nan,
             position_time=math.nan)
    d.update({k: 0 for k in ("rc_dm", "nic", "position_tc", "nic_b", "position_supp", "version", "nic_a", "nic_c", "category",
                             "n_es", "n_position", "nac_v", "velocity_flags", "has")})
    return d


def record(d):
    out = np.zeros(1, dtype=MODEL_DTYPE)
    for k, name in enumerate(BLOCKS):
        if d["blocks"][k] is not None:
            out[name][0] = d["blocks"][k]
    out["time"][0] = d["time"]
    for k, v in d.items():
        if k not in ("blocks", "time"):
            out[k][0] = v
    return out[0]


def usable(time, t, max_age_s):
    age = t - time
    return 0.0 <= age <= max_age_s                       # False for NaN


def resolve(a, rec, t, max_age_s, reached=None):
    """The per-frame output (a FRAME_ES_DTYPE tuple) of a COUNTED frame with record rec heard at t, of the aircraft dict a
    as it stands before the frame."""
    has_version = not math.isnan(a["version_time"])
    version = a["version"] if has_version else M.VERSION_UNKNOWN
    if int(rec["state"]) != M.POSITION:
        return (0, 0, version, 0, COUNTED)
    flags, supp = COUNTED | POSITION | (VERSIONED if has_version else 0), 0
    for held, time, bit, stale in ((a["nic_a"], a["nic_a_time"], 1, STALE_A), (a["nic_c"], a["nic_c_time"], 4, STALE_C)):
        if math.isnan(time):
            continue
        if usable(time, t, max_age_s):
            supp |= bit if held & 1 else 0
        else:
            flags |= stale
    if int(rec["present"]) & M.HAS["NIC_B"] and int(rec["nic_b"]) & 1:
        supp |= 2
    tc = int(rec["type_code"])
    nic, rc = integrity(tc, version, supp)
    if reached is not None:
        reached.add(("row", integrity_row(tc, version, supp)))
        reached.update(name for name, bit in (("STALE_A", STALE_A), ("STALE_C", STALE_C)) if flags & bit)
    return (rc, nic, version, supp, flags)


def count(a, rec, out, t):
    """One COUNTED frame applied to the aircraft's dict, in place: rec its record, out its per-frame output"""
    state, present = int(rec["state"]), int(rec["present"])
    a["n_es"] = min(a["n_es"] + 1, U32)
    block = {(M.OPERATIONAL, 0): 0, (M.OPERATIONAL, 1): 1}.get((state, int(rec["subtype"])),
                                                               {M.TARGET_STATE: 2, M.EMERGENCY: 3, M.ACAS_RA: 4}.get(state))
    if block is not None:
        a["blocks"][block], a["time"][block] = np.array(rec, dtype=M.REC_DTYPE), t
    if present & M.HAS["VERSION"]:
        a["version"], a["version_time"] = int(rec["version"]), t
    if present & M.HAS["NIC_A"]:
        a["nic_a"], a["nic_a_time"] = int(rec["nic_a"]), t
    if present & M.HAS["NIC_C"]:
        a["nic_c"], a["nic_c_time"] = int(rec["nic_c"]), t
    if state == M.CATEGORY:
        a["category"] = int(rec["category"])
    if present & M.HAS["NAC_V"]:
        velocity = state == M.VELOCITY
        a["nac_v"], a["velocity_flags"], a["has"] = int(rec["nac_v"]), (int(rec["flags"]) & 0xFF if velocity else 0), (3 if velocity else 1)
    if state == M.POSITION:
        a["n_position"] = min(a["n_position"] + 1, U32)
        a["rc_dm"], a["nic"] = out[0], out[1]
        a["position_supp"] = out[3] | (out[4] & (VERSIONED | STALE_A | STALE_C)) << 1     # how it was resolved
        a["position_tc"], a["position_time"] = int(rec["type_code"]), t
        a["nic_b"] = int(rec["nic_b"]) if present & M.HAS["NIC_B"] else 0


class Table:
    """The table as the header defines it: {address: side-record dict}, admitted in ascending address per update while
    there is room.  recs None: the plain path, every frame keyed by bytes[1..3]; recs given: the keyed path, a frame
    counts only if its record is SELF or KNOWN."""

    def __init__(self, max_aircraft=65536, seconds_per_sample=0.5e-6, max_age_s=60.0):
        self.state, self.cap, self.sps, self.max_age_s, self.reached = {}, max_aircraft, seconds_per_sample, max_age_s, set()

    def update(self, frames, es=None, recs=None, sample_base=0):
        """update_es (es given) or any other update (None: only admission moves) -> frame_es (FRAME_ES_DTYPE), or None"""
        n = len(frames)
        ok = [recs is None or int(recs[j]["kind"]) in (SELF, KNOWN) for j in range(n)]
        addr = [int.from_bytes(frames["bytes"][j][1:4].tobytes(), "big") if recs is None else int(recs[j]["address"]) & 0xFFFFFF
                for j in range(n)]
        new = sorted({addr[j] for j in range(n) if ok[j]} - set(self.state))
        for a in new[:self.cap - len(self.state)]:
            self.state[a] = empty()
        if es is None:
            return None
        out = np.zeros(n, dtype=FRAME_ES_DTYPE)
        for j in range(n):
            if not ok[j] or addr[j] not in self.state or int(es[j]["state"]) in (M.NOT_ES, M.FOREIGN):
                continue
            t = float(sample_base + int(frames["offset"][j])) * self.sps
            a = self.state[addr[j]]
            o = resolve(a, es[j], t, self.max_age_s, self.reached)
            out[j] = o
            count(a, es[j], o, t)
        return out

    def expire(self, addresses):
        for a in addresses:
            del self.state[a]

    def reset(self):
        self.state = {}

    def records(self):
        """The side records in ascending address, as fetch_es returns them"""
        out = np.zeros(len(self.state), dtype=MODEL_DTYPE)
        for k, a in enumerate(sorted(self.state)):
            out[k] = record(self.state[a])
        return out


def same_records(got, want, what=""):
    got = np.ascontiguousarray(got)
    assert got.dtype.itemsize == 256 and len(got) == len(want), (what, len(got), len(want))
    if got.tobytes() != want.tobytes():
        g = got.view(MODEL_DTYPE)
        bad = [k for k in range(len(want)) if g[k].tobytes() != want[k].tobytes()][:4]
        raise AssertionError((what, [(k, g[k], want[k]) for k in bad]))


def same_frames(got, want, what=""):
    got = np.ascontiguousarray(got)
    assert got.dtype.itemsize == 8 and len(got) == len(want), (what, len(got), len(want))
    if got.tobytes() != want.tobytes():
        g = got.view(FRAME_ES_DTYPE)
        bad = [k for k in range(len(want)) if g[k].tobytes() != want[k].tobytes()][:8]
        raise AssertionError((what, [(k, g[k], want[k]) for k in bad]))
