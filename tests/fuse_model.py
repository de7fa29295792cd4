"""The fused view of a track bank (adsb_track_bank_fuse) restated in NumPy from the rules in include/adsb_hip.h, for the
tests to judge the device by.  It takes what TrackBank.aircraft(), last_heard() and velocity() return and never calls a
fused entry point.

A record of receiver r contributes iff last_heard >= since.  One output record per ICAO with a contributing record,
ascending ICAO.  Every quantity is copied whole from one record: the one with the greatest time among the records that
have the quantity, and among equal times the lowest receiver."""
import numpy as np

from tests.velocity_traffic import MODEL_DTYPE as VELOCITY

NONE = 0xFFFF
# the 128-byte adsb_fused_aircraft layout, written out here so the model does not depend on the library
MODEL_DTYPE = np.dtype([("latitude", "<f8"), ("longitude", "<f8"), ("position_time", "<f8"), ("last_contact", "<f8"),
                        ("last_heard", "<f8"), ("n_frames", "<u8"), ("icao", "<u4"), ("altitude", "<i4"),
                        ("n_receivers", "<u2"), ("heard_receiver", "<u2"), ("contact_receiver", "<u2"),
                        ("position_receiver", "<u2"), ("callsign_receiver", "<u2"), ("velocity_receiver", "<u2"),
                        ("has_position", "<u4"), ("callsign", "S8"), ("velocity", VELOCITY), ("reserved", "<u8", (2,))])
OFFSETS = {"latitude": 0, "longitude": 8, "position_time": 16, "last_contact": 24, "last_heard": 32, "n_frames": 40,
           "icao": 48, "altitude": 52, "n_receivers": 56, "heard_receiver": 58, "contact_receiver": 60,
           "position_receiver": 62, "callsign_receiver": 64, "velocity_receiver": 66, "has_position": 68,
           "callsign": 72, "velocity": 80, "reserved": 112}


def _newest(cands, time, has=lambda c: True):
    """The candidate with the greatest time among those that have the quantity; cands come in ascending receiver
    order and only a strictly greater time replaces the holder, so a tie stays with the lowest receiver."""
    best = None
    for c in cands:
        if has(c) and (best is None or time(c) > time(best)):
            best = c
    return best


def fuse(records, last_heard, velocity, since=-np.inf):
    """records / last_heard / velocity: one array per receiver, aligned (TrackBank.aircraft()[0], .last_heard(),
    .velocity()).  Returns the fused MODEL_DTYPE array."""
    by_icao = {}
    for r, (recs, heard, vels) in enumerate(zip(records, last_heard, velocity)):
        assert len(recs) == len(heard) == len(vels), r
        for rec, lh, v in zip(recs, heard, vels):
            if lh >= since:
                by_icao.setdefault(int(rec["icao"]), []).append((r, rec, float(lh), v))
    out = np.zeros(len(by_icao), dtype=MODEL_DTYPE)
    for k, icao in enumerate(sorted(by_icao)):
        cands, o = by_icao[icao], out[k]
        o["icao"] = icao
        o["n_receivers"] = len(cands)
        o["n_frames"] = sum(int(c[1]["n_frames"]) for c in cands)
        for name in ("contact_receiver", "position_receiver", "callsign_receiver", "velocity_receiver"):
            o[name] = NONE
        o["last_contact"] = o["position_time"] = o["velocity"]["time"] = np.nan
        r, rec, lh, v = _newest(cands, lambda c: c[2])
        o["heard_receiver"], o["last_heard"] = r, lh
        best = _newest(cands, lambda c: c[1]["last_contact"], lambda c: not np.isnan(c[1]["last_contact"]))
        if best is not None:
            o["contact_receiver"], o["last_contact"], o["altitude"] = best[0], best[1]["last_contact"], best[1]["altitude"]
        best = _newest(cands, lambda c: c[1]["last_contact"], lambda c: c[1]["has_position"] != 0)
        if best is not None:
            o["position_receiver"], o["has_position"] = best[0], 1
            o["latitude"], o["longitude"] = best[1]["latitude"], best[1]["longitude"]
            o["position_time"] = best[1]["last_contact"]
        best = _newest(cands, lambda c: c[2], lambda c: c[1]["callsign"] != b"")
        if best is not None:
            o["callsign_receiver"], o["callsign"] = best[0], best[1]["callsign"]
        best = _newest(cands, lambda c: c[3]["time"], lambda c: c[3]["subtype"] != 0)
        if best is not None:
            o["velocity_receiver"], o["velocity"] = best[0], best[3]
    return out
