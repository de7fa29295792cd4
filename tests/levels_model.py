"""NumPy model of the per-frame power statistics (include/adsb_hip.h, adsb_frame_level): the definition restated, the
yardstick of tests/test_levels_host.py and tests/test_gpu_levels.py.  Its dtype is written out here, not imported."""
import numpy as np

MODEL_DTYPE = np.dtype([("signal_sum", "<u8"), ("noise_sum", "<u8"), ("peak", "<u4"), ("pulse_min", "<u4"),
                        ("quiet_max", "<u4"), ("weak_bits", "<u2"), ("flags", "<u2")])
OFFSETS = {"signal_sum": 0, "noise_sum": 8, "peak": 16, "pulse_min": 20, "quiet_max": 24, "weak_bits": 28, "flags": 30}
BITS = np.arange(112)


def levels(iq, frames, first_sample=0):
    """One MODEL_DTYPE record per frame: iq is one channel, (n, 2) int8 / int16, whose sample 0 is stream sample
    first_sample; frames carry `offset` and `bytes`.  (All frames of a block at once: rows = frames.)"""
    iq = np.asarray(iq).reshape(-1, 2).astype(np.int64)
    p = iq[:, 0] ** 2 + iq[:, 1] ** 2
    out = np.zeros(len(frames), dtype=MODEL_DTYPE)
    w = np.array([int(o) - int(first_sample) for o in frames["offset"]], dtype=object)    # exact, may be negative
    ok = np.array([0 <= x and x + 240 <= len(p) for x in w], dtype=bool)                  # else: flags 0, zeros
    for a in range(0, len(frames), 4096):
        rows = np.nonzero(ok[a:a + 4096])[0] + a
        if not len(rows):
            continue
        win = p[w[rows].astype(np.int64)[:, None] + np.arange(240)]                       # [rows, 240]
        bit = np.unpackbits(np.ascontiguousarray(frames["bytes"][rows]), axis=1).astype(np.int64)  # MSB first
        hi, lo = 16 + 2 * BITS + (1 - bit), 16 + 2 * BITS + bit                           # bit 1: the pulse comes first
        pulse = np.zeros(win.shape, dtype=bool)
        pulse[:, [0, 2, 7, 9]] = True
        np.put_along_axis(pulse, hi, True, axis=1)
        assert (pulse.sum(axis=1) == 116).all()
        p_hi, p_lo = np.take_along_axis(win, hi, axis=1), np.take_along_axis(win, lo, axis=1)
        out["signal_sum"][rows] = np.where(pulse, win, 0).sum(axis=1)
        out["noise_sum"][rows] = np.where(pulse, 0, win).sum(axis=1)
        out["peak"][rows] = win.max(axis=1)
        out["pulse_min"][rows] = np.where(pulse, win, 1 << 40).min(axis=1)
        out["quiet_max"][rows] = np.where(pulse, -1, win).max(axis=1)
        out["weak_bits"][rows] = (p_hi < 2 * p_lo).sum(axis=1)
        out["flags"][rows] = 1
    return out
