"""Independent model of a track table's Mode S side (include/adsb_hip.h, "Mode S replies per aircraft"), written from the
definitions in plain Python: a dict per aircraft and a sequential loop over the frames, the way a transponder's replies
arrive.  Calls no library entry point.  Shared by the CPU and GPU tiers.

The model covers what update_modes adds: which frames are accepted, which aircraft a list admits, every frame's point
flags and icao, and the 64-byte side record.  The main 128-byte record is checked differently (tests/
test_gpu_track_modes.py): against adsb_track_table_update on a transformed list, which is the definition the header
gives for it."""
import numpy as np

SELF, KNOWN, UNKNOWN, PARITY, UNSUPPORTED = range(5)
M_ALT, M_SQUAWK, M_GROUND, M_ALERT, M_SPI, M_CALLSIGN = 0x1, 0x4, 0x8, 0x10, 0x20, 0x40     # adsb_modes_rec.flags
ALT, SQUAWK, GROUND, ALERT, SPI, CALLSIGN, STATUS, SQUITTER = 0x1, 0x4, 0x8, 0x10, 0x20, 0x40, 0x100, 0x200
NEW_POSITION, UNTRACKED, UNADDRESSED = 0x1, 0x2, 0x4                                      # adsb_track_point.flags
TABLE_FULL = 0x1
U32 = 2 ** 32 - 1
SURVEILLANCE_DFS, AIRAIR_DFS = (4, 5, 20, 21), (0, 16)

MODEL_DTYPE = np.dtype([("altitude_time", "<f8"), ("squawk_time", "<f8"), ("callsign_time", "<f8"),
                        ("altitude_ft", "<i4"), ("squawk", "<u2"), ("flags", "<u2"), ("callsign", "S8"),
                        ("n_replies", "<u4"), ("n_allcall", "<u4"), ("n_surveillance", "<u4"), ("n_airair", "<u4"),
                        ("fs", "u1"), ("last_df", "u1"), ("reserved", "u1", (6,))])
OFFSETS = {"altitude_time": 0, "squawk_time": 8, "callsign_time": 16, "altitude_ft": 24, "squawk": 28, "flags": 30,
           "callsign": 32, "n_replies": 40, "n_allcall": 44, "n_surveillance": 48, "n_airair": 52, "fs": 56,
           "last_df": 57, "reserved": 58}
assert MODEL_DTYPE.itemsize == 64 and all(MODEL_DTYPE.fields[k][1] == v for k, v in OFFSETS.items())
COUNTS = ("n_replies", "n_allcall", "n_surveillance", "n_airair")


def empty():
    """The EMPTY record as a dict: zeros, the three times NaN."""
    return dict(altitude_time=np.nan, squawk_time=np.nan, callsign_time=np.nan, altitude_ft=0, squawk=0, flags=0,
                callsign=b"", n_replies=0, n_allcall=0, n_surveillance=0, n_airair=0, fs=0, last_df=0)


def record(d):
    """A dict -> its 64 bytes as a MODEL_DTYPE record."""
    out = np.zeros(1, dtype=MODEL_DTYPE)
    for k, v in d.items():
        out[k][0] = v
    return out[0]


def as_dict(rec):
    """A MODEL_DTYPE (or AIRCRAFT_MODES_DTYPE) record -> the dict; callsign keeps its bytes as numpy gives them."""
    return {k: (bytes(rec[k]) if k == "callsign" else rec[k].item()) for k in MODEL_DTYPE.names if k != "reserved"}


def accepted(rec):
    return int(rec["kind"]) in (SELF, KNOWN)


def count(a, rec, time):
    """One COUNTED frame applied to the aircraft's dict `a`, in place."""
    df, flags = int(rec["df"]), int(rec["flags"])
    if df in (17, 18):
        a["flags"] |= SQUITTER
    else:
        a["n_replies"] = min(a["n_replies"] + 1, U32)
        if df == 11:
            a["n_allcall"] = min(a["n_allcall"] + 1, U32)
        if df in SURVEILLANCE_DFS:
            a["n_surveillance"] = min(a["n_surveillance"] + 1, U32)
        if df in AIRAIR_DFS:
            a["n_airair"] = min(a["n_airair"] + 1, U32)
    a["last_df"] = df
    if flags & M_ALT:
        a["altitude_ft"], a["altitude_time"] = int(rec["altitude_ft"]), time
        a["flags"] |= ALT
    if flags & M_SQUAWK:
        a["squawk"], a["squawk_time"] = int(rec["squawk"]), time
        a["flags"] |= SQUAWK
    if flags & M_CALLSIGN:
        a["callsign"], a["callsign_time"] = bytes(rec["callsign"]), time
        a["flags"] |= CALLSIGN
    if df in SURVEILLANCE_DFS:
        a["fs"] = int(rec["fs"])
        a["flags"] = (a["flags"] & ~(ALERT | SPI)) | STATUS | (flags & (M_ALERT | M_SPI))
    if df in SURVEILLANCE_DFS + AIRAIR_DFS:
        a["flags"] = (a["flags"] & ~GROUND) | (flags & M_GROUND)
    return a


class Table:
    """The table as the header defines it: {address: side-record dict}, admitted in ascending address per update while
    there is room."""

    def __init__(self, max_aircraft=65536, seconds_per_sample=0.5e-6):
        self.state, self.cap, self.sps, self.flags = {}, max_aircraft, seconds_per_sample, 0

    def update(self, frames, recs, sample_base=0):
        """-> (point flags without NEW_POSITION, point icao), one per frame"""
        n = len(frames)
        ok = [accepted(recs[j]) for j in range(n)]
        addr = [int(recs[j]["address"]) & 0xFFFFFF for j in range(n)]
        new = sorted({addr[j] for j in range(n) if ok[j]} - set(self.state))
        room = self.cap - len(self.state)
        for a in new[:room]:
            self.state[a] = empty()
        if len(new) > room:
            self.flags |= TABLE_FULL
        flags, icao = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
        for j in range(n):
            if not ok[j]:
                flags[j], icao[j] = UNADDRESSED, int(recs[j]["address"])
                continue
            icao[j] = addr[j]
            if addr[j] not in self.state:
                flags[j] = UNTRACKED
                continue
            count(self.state[addr[j]], recs[j], float(sample_base + int(frames["offset"][j])) * self.sps)
        return flags, icao

    def expire(self, last_heard, before):
        """last_heard: {address: time}; evicts every aircraft heard last before `before`"""
        for a in [a for a in self.state if last_heard[a] < before]:
            del self.state[a]

    def records(self):
        """The side records in ascending address, as fetch_modes returns them"""
        out = np.zeros(len(self.state), dtype=MODEL_DTYPE)
        for k, a in enumerate(sorted(self.state)):
            out[k] = record(self.state[a])
        return out


def to_squitters(frames, recs):
    """The transformed list of the differential test: every accepted frame that is no DF17/18 becomes a 14-byte DF17
    frame with bytes[1..3] = address and bytes[4..] = 0 (type code 0: a frame of kind "other") at the same offset,
    accepted DF17/18 frames stay, the rest is dropped.  -> (the list, the indices kept)"""
    keep = [j for j in range(len(frames)) if accepted(recs[j])]
    out = frames[keep].copy()
    for k, j in enumerate(keep):
        if int(recs[j]["df"]) not in (17, 18):
            a = int(recs[j]["address"]) & 0xFFFFFF
            out["bytes"][k] = 0
            out["bytes"][k][:4] = (17 << 3, a >> 16, (a >> 8) & 0xFF, a & 0xFF)
    return out, np.array(keep, dtype=np.int64)


def same_records(got, want, what=""):
    got = np.ascontiguousarray(got)
    assert got.dtype.itemsize == 64 and len(got) == len(want), (what, len(got), len(want))
    if got.tobytes() != want.tobytes():
        g = got.view(MODEL_DTYPE)
        bad = [k for k in range(len(want)) if g[k].tobytes() != want[k].tobytes()][:4]
        raise AssertionError((what, [(k, g[k], want[k]) for k in bad]))
