"""The CPU mirror's functions put together the way the device puts its kernels together: per update, every counted frame
is settled (adsb_host_commb_settle) against the aircraft's newest earlier velocity message (adsb_host_commb_reference of
a frame of this list, else the one held), the frames' contributions (adsb_host_track_commb_of) are folded into one part
per aircraft and the part is merged into the record (adsb_host_track_commb_merge).  Admission is the model's rule."""
import numpy as np

import air_rs_amd as A
from tests import track_commb_model as T


class Table:
    def __init__(self, max_aircraft=65536, seconds_per_sample=0.5e-6, cfg=None):
        self.state, self.cap, self.sps = {}, max_aircraft, seconds_per_sample
        self.cfg = dict(T.DEFAULT_CFG, **(cfg or {}))

    def update(self, frames, recs, commb, sample_base=0):
        n = len(frames)
        ok = [int(recs[j]["kind"]) in (T.SELF, T.KNOWN) for j in range(n)]
        addr = [int(recs[j]["address"]) & 0xFFFFFF for j in range(n)]
        new = sorted({addr[j] for j in range(n) if ok[j]} - set(self.state))
        empty = A.host_track_commb_of(np.zeros(1, dtype=A.COMMB_DTYPE)[0])
        for a in new[:self.cap - len(self.state)]:
            self.state[a] = dict(rec=empty.copy(), vel=None)
        out, parts = np.array(commb, dtype=A.COMMB_DTYPE), {}
        for j in range(n):
            if not ok[j] or addr[j] not in self.state:
                continue
            a, b = self.state[addr[j]], frames["bytes"][j].tobytes()
            t = float(sample_base + int(frames["offset"][j])) * self.sps
            if int(commb[j]["state"]) != T.NOT_COMMB:
                out[j] = A.host_commb_settle(b, commb[j], a["vel"], t, **self.cfg)
                one = A.host_track_commb_of(out[j], t)
                parts[addr[j]] = A.host_track_commb_merge(parts[addr[j]], one) if addr[j] in parts else one
            if int(recs[j]["df"]) in (17, 18) and b[4] >> 3 == 19:
                v = A.host_commb_reference(b, t)
                if int(v["subtype"]):
                    a["vel"] = v
        for k, part in parts.items():
            self.state[k]["rec"] = A.host_track_commb_merge(self.state[k]["rec"], part)
        return out

    def records(self):
        out = np.zeros(len(self.state), dtype=A.AIRCRAFT_COMMB_DTYPE)
        for k, a in enumerate(sorted(self.state)):
            out[k] = self.state[a]["rec"]
        return out


def run(case, cuts=(), **table):
    t = Table(**table)
    edges = [0] + list(cuts) + [len(case["frames"])]
    outs = [t.update(case["frames"][a:b], case["recs"][a:b], case["commb"][a:b]) for a, b in zip(edges, edges[1:])]
    return np.concatenate(outs) if outs else np.zeros(0, dtype=A.COMMB_DTYPE), t.records()
