"""The replies scan (include/adsb_hip.h, "Mode S replies from samples") as a NumPy model, written from the definition in
the header text and independent of air_rs_amd/csrc/adsb_replies.h: power, the strict preamble test over every examined
offset at once, then the few candidates one by one (DF, window, slicer, syndrome by modes_model.crc24's long division,
the decision), the list with its capacity, the counts and the header; the stable merge of two lists; and the renderer
the cases use: Mode S messages as PPM pulses over seeded noise, int8 or int16."""
import numpy as np

from tests import modes_model as MM

FRAME_DTYPE = MM.FRAME_DTYPE
HEADER_FIELDS = ("n_out", "total_found", "n_preamble", "n_all_call", "n_df18", "n_address_parity", "n_not_known", "n_parity",
                 "flags", "reserved")
HEADER_DTYPE = np.dtype([(k, "<u8") for k in HEADER_FIELDS])
PULSES = (0, 2, 7, 9)
GAPS = (1, 3, 4, 5, 6, 8, 10, 11, 12, 13, 14, 15)
ADDRESS_PARITY = (0, 4, 5, 16, 20, 21)
TRUNCATED = 1
FROM_B = 0x80000000


def power(iq):
    s = np.asarray(iq).reshape(-1, 2).astype(np.int64)
    return s[:, 0] ** 2 + s[:, 1] ** 2


def message_at(p, i):
    """(DF, bit count L, the L bits sliced at offset i or None if the frame does not fit)"""
    n = len(p)
    head = p[i + 16:i + 26:2] > p[i + 17:i + 26:2]
    df = int("".join("01"[int(b)] for b in head), 2)
    nbits = 56 if df < 16 else 112
    if i + 16 + 2 * nbits > n:
        return df, nbits, None
    return df, nbits, p[i + 16:i + 16 + 2 * nbits:2] > p[i + 17:i + 16 + 2 * nbits:2]


def channel(p, known, ap_known):
    """One channel's powers -> (list of (offset, 14 bytes) kept, the six counts)"""
    n = len(p)
    tally = dict.fromkeys(HEADER_FIELDS[2:8], 0)
    kept = []
    m = n - 25                                     # offsets examined: i + 26 <= n
    if m <= 0:
        return kept, tally
    win = np.lib.stride_tricks.sliding_window_view(p, 16)[:m]
    pre = win[:, PULSES].min(axis=1) > win[:, GAPS].max(axis=1)
    for i in np.nonzero(pre)[0]:
        i = int(i)
        tally["n_preamble"] += 1
        df, nbits, bits = message_at(p, i)
        if df not in ADDRESS_PARITY + (11, 18) or bits is None:
            continue
        msg = np.packbits(bits).tobytes()
        s = MM.crc24(msg[:-3]) ^ int.from_bytes(msg[-3:], "big")
        if df == 11:
            what = "n_all_call" if s < 128 else "n_parity"
        elif df == 18:
            what = "n_df18" if s == 0 else "n_parity"
        else:
            what = "n_not_known" if ap_known and s not in known else "n_address_parity"
        tally[what] += 1
        if what in ("n_all_call", "n_df18", "n_address_parity"):
            kept.append((i, msg + bytes(14 - len(msg))))
    return kept, tally


def replies(iq, n_channels=1, n_samples=None, channel_stride=None, known=None, ap="all", max_frames=0, first_sample=0):
    """-> (FRAME_DTYPE frames, uint64 counts, HEADER_DTYPE record): the arguments of AdsbDemod.replies_of /
    host_replies; max_frames = 0 is no limit."""
    p = power(iq)
    n_samples = len(p) // n_channels if n_samples is None else n_samples
    stride = n_samples if channel_stride is None else channel_stride
    known = set() if known is None else set(int(a) for a in known)
    total = dict.fromkeys(HEADER_FIELDS[2:8], 0)
    rows, counts = [], []
    for c in range(n_channels):
        kept, tally = channel(p[c * stride:c * stride + n_samples], known, ap == "known")
        for k in tally:
            total[k] += tally[k]
        rows.append(kept)
        counts.append(len(kept))
    found = sum(counts)
    cap = found if max_frames == 0 else max_frames
    frames = np.zeros(min(found, cap), dtype=FRAME_DTYPE)
    at, clipped = 0, []
    for kept in rows:
        room = max(min(len(kept), len(frames) - at), 0)
        for i, msg in kept[:room]:
            frames[at]["offset"] = first_sample + i
            frames[at]["bytes"] = np.frombuffer(msg, dtype=np.uint8)
            frames[at]["fixed_bit"] = 0xFF
            at += 1
        clipped.append(room)
    hdr = np.zeros((), dtype=HEADER_DTYPE)
    hdr["n_out"], hdr["total_found"] = len(frames), found
    for k in total:
        hdr[k] = total[k]
    hdr["flags"] = TRUNCATED if found > cap else 0
    return frames, np.array(clipped, dtype=np.uint64), hdr


def merge(a, counts_a, b, counts_b):
    """The stable merge, channel by channel: ascending offset, a's frame first on equal offsets -> (frames, src, counts)"""
    out, src, counts, pa, pb = [], [], [], 0, 0
    for ca, cb in zip(counts_a, counts_b):
        ca, cb = int(ca), int(cb)
        rows = [(int(a[pa + k]["offset"]), 0, pa + k) for k in range(ca)] + [(int(b[pb + k]["offset"]), 1, pb + k) for k in range(cb)]
        for _, which, k in sorted(rows):              # (offset, list, index): python's tuple order is the rule
            out.append((b if which else a)[k])
            src.append(k | (FROM_B if which else 0))
        counts.append(ca + cb)
        pa, pb = pa + ca, pb + cb
    frames = np.array(out, dtype=FRAME_DTYPE) if out else np.zeros(0, dtype=FRAME_DTYPE)
    return frames, np.array(src, dtype=np.uint32), np.array(counts, dtype=np.uint64)


# ---- rendering -------------------------------------------------------------------------------------------------------
def noise(n, dtype, seed, span):
    """n samples of seeded noise, I and Q uniform in [-span, span]"""
    rng = np.random.default_rng(seed)
    return rng.integers(-span, span + 1, size=(n, 2)).astype(dtype)


def pulse_positions(msg, at):
    """sample indices of the pulses of one message rendered at offset `at`"""
    bits = np.unpackbits(np.frombuffer(bytes(msg), dtype=np.uint8))
    return [at + k for k in PULSES] + [at + 16 + 2 * k + (0 if b else 1) for k, b in enumerate(bits)]


def render(iq, msg, at, pulse=(100, 0)):
    """msg as PPM pulses of value `pulse` into iq (a flat [samples, 2] array); pulses past the end are dropped"""
    for s in pulse_positions(msg, at):
        if 0 <= s < len(iq):
            iq[s] = pulse
    return iq
