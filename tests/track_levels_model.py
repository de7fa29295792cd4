"""Per-aircraft signal levels of a track table / bank (adsb_aircraft_level) and the fused levels of a bank
(adsb_fused_level), restated in Python from the rules in include/adsb_hip.h, for the tests to judge the device by.  The
dtypes are written out here, not imported from the library; the arithmetic is Python integers clamped at 2^64 - 1 and
2^32 - 1; no level entry point of a store is ever called.

Frame j of an update is COUNTED for its aircraft iff its point is not UNTRACKED and levels[j].flags has bit 0.  Over the
counted frames: totals and the count are saturating sums, max_signal_sum and peak maxima, last_* those of the newest
counted frame (the last one in list order), last_time = float(sample_base + offset) * seconds_per_sample, one rounded
product.  An empty record is zeros with last_time NaN."""
import math

import numpy as np

U64, U32 = (1 << 64) - 1, (1 << 32) - 1
NONE = 0xFFFF
# adsb_frame_level (32 bytes), the input
FRAME_LEVEL = np.dtype([("signal_sum", "<u8"), ("noise_sum", "<u8"), ("peak", "<u4"), ("pulse_min", "<u4"),
                        ("quiet_max", "<u4"), ("weak_bits", "<u2"), ("flags", "<u2")])
# adsb_aircraft_level (64 bytes)
MODEL_DTYPE = np.dtype([("signal_total", "<u8"), ("noise_total", "<u8"), ("last_signal_sum", "<u8"),
                        ("last_noise_sum", "<u8"), ("max_signal_sum", "<u8"), ("last_time", "<f8"), ("n_levels", "<u4"),
                        ("peak", "<u4"), ("weak_bits_total", "<u4"), ("reserved", "<u4")])
OFFSETS = {"signal_total": 0, "noise_total": 8, "last_signal_sum": 16, "last_noise_sum": 24, "max_signal_sum": 32,
           "last_time": 40, "n_levels": 48, "peak": 52, "weak_bits_total": 56, "reserved": 60}
# adsb_fused_level (96 bytes)
FUSED_DTYPE = np.dtype([("strongest", MODEL_DTYPE), ("signal_total", "<u8"), ("noise_total", "<u8"), ("n_levels", "<u8"),
                        ("strongest_receiver", "<u2"), ("level_receivers", "<u2"), ("reserved", "<u4")])
FUSED_OFFSETS = {"strongest": 0, "signal_total": 64, "noise_total": 72, "n_levels": 80, "strongest_receiver": 88,
                 "level_receivers": 90, "reserved": 92}


def empty():
    return {"signal_total": 0, "noise_total": 0, "last_signal_sum": 0, "last_noise_sum": 0, "max_signal_sum": 0,
            "last_time": math.nan, "n_levels": 0, "peak": 0, "weak_bits_total": 0, "reserved": 0}


def frame_icaos(frames):
    b = frames["bytes"].astype(np.int64)
    return (b[:, 1] << 16) | (b[:, 2] << 8) | b[:, 3]


def apply(state, frames, levels, sample_base=0, sps=0.5e-6, untracked=None):
    """One update: merges the list into state (dict ICAO -> level dict), frame by frame in list order.  untracked: a
    bool per frame, True where the store turned the frame's aircraft away (its point has ADSB_TRACK_UNTRACKED)."""
    assert len(frames) == len(levels)
    for j, icao in enumerate(frame_icaos(frames)):
        if untracked is not None and untracked[j]:
            continue
        if not int(levels[j]["flags"]) & 1:
            continue
        a = state.setdefault(int(icao), empty())
        sig, noise = int(levels[j]["signal_sum"]), int(levels[j]["noise_sum"])
        a["signal_total"] = min(a["signal_total"] + sig, U64)
        a["noise_total"] = min(a["noise_total"] + noise, U64)
        a["last_signal_sum"], a["last_noise_sum"] = sig, noise
        a["max_signal_sum"] = max(a["max_signal_sum"], sig)
        a["last_time"] = float(int(sample_base) + int(frames[j]["offset"])) * sps
        a["n_levels"] = min(a["n_levels"] + 1, U32)
        a["peak"] = max(a["peak"], int(levels[j]["peak"]))
        a["weak_bits_total"] = min(a["weak_bits_total"] + int(levels[j]["weak_bits"]), U32)
    return state


def records(state, icaos):
    """The MODEL_DTYPE array for the aircraft `icaos` (the order of the store's fetch); an aircraft the model has no
    counted frame for is empty."""
    out = np.zeros(len(icaos), dtype=MODEL_DTYPE)
    for k, icao in enumerate(icaos):
        for name, v in state.get(int(icao), empty()).items():
            out[k][name] = v
    return out


def stronger(a, b):
    """a's mean signal is strictly greater than b's, exactly (both with n_levels > 0)."""
    return int(a["signal_total"]) * int(b["n_levels"]) > int(b["signal_total"]) * int(a["n_levels"])


def fuse(icaos, last_heard, levels, since=-math.inf):
    """icaos / last_heard / levels: one array per receiver, aligned (the records' ICAOs, their last-heard times, their
    MODEL_DTYPE level records).  One FUSED_DTYPE record per ICAO with a contributing record (last_heard >= since),
    ascending ICAO; a caller that models truncation keeps the first max_fused."""
    by_icao = {}
    for r, (ic, lh, lv) in enumerate(zip(icaos, last_heard, levels)):
        assert len(ic) == len(lh) == len(lv), r
        for icao, t, a in zip(ic, lh, lv):
            if t >= since:
                by_icao.setdefault(int(icao), []).append((r, a))
    out = np.zeros(len(by_icao), dtype=FUSED_DTYPE)
    for k, icao in enumerate(sorted(by_icao)):
        o, best = out[k], None
        sig = noise = n = heard = 0
        for r, a in by_icao[icao]:                       # receivers ascending: only a strictly greater mean replaces
            sig, noise = min(sig + int(a["signal_total"]), U64), min(noise + int(a["noise_total"]), U64)
            n += int(a["n_levels"])
            if int(a["n_levels"]) == 0:
                continue
            heard += 1
            if best is None or stronger(a, best[1]):
                best = (r, a)
        o["signal_total"], o["noise_total"], o["n_levels"], o["level_receivers"] = sig, noise, n, heard
        if best is None:
            o["strongest"], o["strongest_receiver"] = records({}, [0])[0], NONE
        else:
            o["strongest"], o["strongest_receiver"] = best[1], best[0]
    return out
