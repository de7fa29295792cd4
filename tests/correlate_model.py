"""An independent model of correlate (include/adsb_hip.h, "Correlate") for the tests: pure Python over tuples
(K as int, T, j), sorted and walked, straight from the definitions.  Its own dtype tables; calls no library entry point.

  reception j: list index j of receiver r(j); T = (sample_base[r] + offset) mod 2^64; K = the 14 bytes, big-endian
  group order: (K, T, j) ascending
  head: first in group order, another K than the predecessor, or T - T_pred > window
  message: one per group, time = T of the group's first reception; messages in ascending (time, K)
  receptions: message by message, (T, j) inside a message
"""
import numpy as np

FRAME_DTYPE = np.dtype([("offset", "<u8"), ("bytes", "u1", (14,)), ("status", "u1"), ("fixed_bit", "u1")])
LEVEL_DTYPE = np.dtype([("signal_sum", "<u8"), ("noise_sum", "<u8"), ("peak", "<u4"), ("pulse_min", "<u4"),
                        ("quiet_max", "<u4"), ("weak_bits", "<u2"), ("flags", "<u2")])
MESSAGE_DTYPE = np.dtype({
    "names": ["time", "bytes", "status", "fixed_bit", "first", "n_receptions", "n_receivers", "first_receiver",
              "best_receiver", "reserved", "n_clean", "reserved2", "span", "best_signal_sum"],
    "formats": ["<u8", ("u1", (14,)), "u1", "u1", "<u4", "<u4", "<u2", "<u2", "<u2", "<u2", "<u4", "<u4", "<u8", "<u8"],
    "offsets": [0, 8, 22, 23, 24, 28, 32, 34, 36, 38, 40, 44, 48, 56],
    "itemsize": 64})
RECEPTION_DTYPE = np.dtype({"names": ["time", "frame", "receiver", "reserved"], "formats": ["<u8", "<u4", "<u2", "<u2"],
                            "offsets": [0, 8, 12, 14], "itemsize": 16})
LEVEL_VALID = 1
NO_RECEIVER = 0xFFFF
MAX_RECEIVERS = 256
M64 = (1 << 64) - 1


def correlate(frames, counts, window, sample_base=None, levels=None):
    """(messages, frames_out, receptions) as MESSAGE_DTYPE, FRAME_DTYPE and RECEPTION_DTYPE arrays."""
    n = len(frames)
    counts = [int(c) for c in counts]
    assert 1 <= len(counts) <= MAX_RECEIVERS and sum(counts) == n and 0 <= int(window) < (1 << 32)
    base = [0] * len(counts) if sample_base is None else [int(b) for b in sample_base]
    receiver = [r for r, c in enumerate(counts) for _ in range(c)]
    rows = []
    for j in range(n):
        t = (base[receiver[j]] + int(frames["offset"][j])) & M64
        rows.append((int.from_bytes(frames["bytes"][j].tobytes(), "big"), t, j))
    rows.sort()
    groups = []
    for k, (key, t, j) in enumerate(rows):
        if k == 0 or rows[k - 1][0] != key or t - rows[k - 1][1] > int(window):
            groups.append([])
        groups[-1].append((key, t, j))
    groups.sort(key=lambda g: (g[0][1], g[0][0]))

    msgs = np.zeros(len(groups), dtype=MESSAGE_DTYPE)
    fout = np.zeros(len(groups), dtype=FRAME_DTYPE)
    recs = np.zeros(n, dtype=RECEPTION_DTYPE)
    q = 0
    for m, g in enumerate(groups):
        key, time, _ = g[0]
        status = min(int(frames["status"][j]) for _, _, j in g)
        holder = next(j for _, _, j in g if int(frames["status"][j]) == status)
        best, best_sum = NO_RECEIVER, 0
        if levels is not None:
            for _, _, j in g:
                if int(levels["flags"][j]) & LEVEL_VALID and (best == NO_RECEIVER or int(levels["signal_sum"][j]) > best_sum):
                    best, best_sum = receiver[j], int(levels["signal_sum"][j])
        msgs[m] = (time, np.frombuffer(key.to_bytes(14, "big"), dtype=np.uint8), status, int(frames["fixed_bit"][holder]),
                   q, len(g), len({receiver[j] for _, _, j in g}), receiver[g[0][2]], best, 0,
                   sum(1 for _, _, j in g if int(frames["status"][j]) == 0), 0, g[-1][1] - time, best_sum)
        fout[m] = (time, msgs["bytes"][m], status, int(frames["fixed_bit"][holder]))
        for _, t, j in g:
            recs[q] = (t, j, receiver[j], 0)
            q += 1
    assert q == n
    return msgs, fout, recs


def same(got, want, what=""):
    """Byte-for-byte comparison of two (messages, frames, receptions) results, with a readable first difference."""
    for name, g, w in zip(("messages", "frames", "receptions"), got, want):
        assert g.dtype.itemsize == w.dtype.itemsize, (what, name, g.dtype.itemsize, w.dtype.itemsize)
        assert len(g) == len(w), (what, name, len(g), len(w))
        if g.tobytes() != w.tobytes():
            k = next(i for i in range(len(g)) if g[i].tobytes() != w[i].tobytes())
            raise AssertionError((what, name, k, g[k], w[k]))


# ---- lists ----------------------------------------------------------------------------------------------------------------
def build(per_receiver, levels=False):
    """per_receiver: one list per receiver of (offset, bytes14, status, fixed_bit[, signal_sum, level flags]) in any
    order; sorted by offset per receiver (stable) -> (frames, counts[, levels])."""
    rows = [row for rx in per_receiver for row in sorted(rx, key=lambda row: row[0])]
    fr = np.zeros(len(rows), dtype=FRAME_DTYPE)
    lv = np.zeros(len(rows), dtype=LEVEL_DTYPE)
    for k, row in enumerate(rows):
        fr[k] = (int(row[0]) & M64, np.frombuffer(bytes(row[1]), dtype=np.uint8), row[2], row[3])
        if len(row) > 4:
            lv[k]["signal_sum"], lv[k]["flags"] = row[4], row[5]
    counts = np.array([len(rx) for rx in per_receiver], dtype=np.uint64)
    return (fr, counts, lv) if levels else (fr, counts)


def random_list(n, n_receivers, seed, window=40):
    """n receptions over n_receivers receivers of about n / 3 distinct transmissions, each heard by random receivers at
    times within a few windows of each other (so groups of 1..n_receivers and chains that split occur), random status
    and fixed_bit, random levels (some invalid, some equal).  -> (frames, counts, levels)."""
    rng = np.random.default_rng(seed)
    n_tx = max(n // 3, 1)
    tx_bytes = rng.integers(0, 256, size=(n_tx, 14)).astype(np.uint8)
    tx_time = np.cumsum(rng.integers(1, 4 * window, size=n_tx))
    per = [[] for _ in range(n_receivers)]
    for _ in range(n):
        x, r = int(rng.integers(0, n_tx)), int(rng.integers(0, n_receivers))
        status = int(rng.integers(0, 2))
        per[r].append((int(tx_time[x]) + int(rng.integers(0, 3 * window)), tx_bytes[x].tobytes(), status,
                       int(rng.integers(0, 88)) if status else 0xFF, int(rng.integers(0, 6)) * 1000,
                       int(rng.integers(0, 4) != 0)))
    return build(per, levels=True)
