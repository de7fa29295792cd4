"""The cases of the short-frame output tests (level records by frame length, wire output with ADSB_WIRE_SHORT): sample
buffers with frame lists for the levels, and frame lists with level records for the wire.  The CPU tier runs them
through the mirror and the model, the GPU tier through the device as well."""
import numpy as np

from tests import levels_modes_model as LM
from tests.wire_model import FRAME_DTYPE, LEVEL_DTYPE, I8, I16, smallest_sum_for

LENGTHS = (128, 129, 240, 241, 367)
SHORT_DFS = (0, 4, 5, 11, 15)
LONG_DFS = (16, 17, 20, 24, 25, 26, 27, 28, 29, 30, 31)
TAIL = 256                                # full-scale samples behind the last channel: a read past it stays in the buffer
FIRST = 10 ** 12 + 7                      # first_sample_index of every case
_CASES = {}


def frame(df, offset, rng, fill=None):
    """a frame of that DF with random bytes; fill: what bytes[7..14) of a short frame hold (default zeros)"""
    f = np.zeros((), dtype=FRAME_DTYPE)
    b = rng.integers(0, 256, 14).astype(np.uint8)
    b[0] = df << 3 | int(rng.integers(0, 8))
    if df < 16:
        b[7:] = 0 if fill is None else fill
    f["offset"], f["bytes"], f["fixed_bit"] = offset, b, 0xFF
    return f


def samples(dtype, n_channels, n, rng):
    """n_channels touching channels of n samples over the type's full range, each opening with 16 full-scale samples (so
    a read past a short window that ends at the channel's end, or past the channel, changes a sum), and TAIL more"""
    info = np.iinfo(dtype)
    buf = rng.integers(info.min, info.max + 1, size=(n_channels * n + TAIL, 2)).astype(dtype)
    for c in range(n_channels + 1):
        buf[c * n:c * n + 16] = info.min
    buf[n_channels * n:] = info.min
    return buf


def levels_case(dtype, n):
    """four channels of n samples with stride == n, channel 2 without frames; short frames at 0, 1, n-128, n-127, long
    ones at 0, 1, n-240, n-239 (whichever are not negative), one frame in front of first_sample, every DF of SHORT_DFS
    and LONG_DFS"""
    key = (np.dtype(dtype).name, n)
    if key in _CASES:
        return _CASES[key]
    rng = np.random.default_rng(1000 + n + (7 if np.dtype(dtype) == np.int16 else 0))
    iq = samples(dtype, 4, n, rng)
    frames, counts, k = [], [], 0
    for c in range(4):
        mine = []
        if c != 2:
            # a channel's first and last frame are valid ones (a frame given to the neighbouring channel shows)
            mine.append(frame(SHORT_DFS[c], FIRST, rng))
            mine.append(frame(4, FIRST - 1, rng))
            mine.append(frame(17, FIRST - 1, rng))
            for w in sorted({0, 1, 3 + c, n - 240, n - 239, n - 241}):
                if w >= 0:
                    mine.append(frame(LONG_DFS[k % len(LONG_DFS)], FIRST + w, rng))
                    k += 1
            for w in sorted({1, 2 + c, n - 127, n - 129}):
                if w >= 0:
                    mine.append(frame(SHORT_DFS[k % len(SHORT_DFS)], FIRST + w, rng))
                    k += 1
            mine.append(frame(SHORT_DFS[(c + 1) % len(SHORT_DFS)], FIRST + n - 128, rng))
        frames += mine
        counts.append(len(mine))
    made = dict(name=f"{np.dtype(dtype).name} n={n}", iq=iq, n_channels=4, n_samples=n, stride=n,
                frames=np.array(frames, dtype=FRAME_DTYPE), counts=counts, first=FIRST)
    _CASES[key] = made
    return made


def extremes_case(dtype):
    """one channel of 367 samples that are all (-128, -128) / (-32768, -32768): the largest sums and the largest power"""
    info = np.iinfo(dtype)
    rng = np.random.default_rng(5)
    iq = np.full((367 + TAIL, 2), info.min, dtype=dtype)
    frames = np.array([frame(11, FIRST + 3, rng), frame(17, FIRST + 100, rng), frame(15, FIRST + 239, rng),
                       frame(16, FIRST + 127, rng)], dtype=FRAME_DTYPE)
    return dict(name=f"{np.dtype(dtype).name} extremes", iq=iq, n_channels=1, n_samples=367, stride=367, frames=frames,
                counts=[4], first=FIRST)


def levels_cases(dtype):
    return [levels_case(dtype, n) for n in LENGTHS] + [extremes_case(dtype)]


def model_levels(c):
    if "model" not in c:
        c["model"] = LM.levels(c["iq"], c["frames"], c["counts"], c["n_samples"], c["stride"], c["first"])
    return c["model"]


def check_levels_expectations(c, got):
    """what the case's construction says, whatever model and mirror agree on"""
    n, first = c["n_samples"], c["first"]
    for f, r in zip(c["frames"], got):
        w, short = int(f["offset"]) - first, (int(f["bytes"][0]) >> 3) < 16
        inside = 0 <= w and w + (128 if short else 240) <= n
        assert int(r["flags"]) == ((LM.VALID | (LM.SHORT if short else 0)) if inside else 0), (c["name"], w, short)
        if not inside:
            assert r.tobytes() == bytes(32)


# ---- wire ------------------------------------------------------------------------------------------------------------
def wire_list(n, seed, mix="random", one_in=8, sample_type=I8):
    """n frames at ascending offsets, 0x1A among their bytes now and then, with level records that carry SHORT for the
    short frames and signal bytes all over 0..255 (a few invalid) -> (frames, levels).  mix: "short", "long",
    "alternate" or "random"."""
    rng = np.random.default_rng(seed)
    fr = np.zeros(n, dtype=FRAME_DTYPE)
    fr["offset"] = np.cumsum(rng.integers(1, 3000, size=n)).astype(np.uint64)
    b = rng.integers(0, 256, size=(n, 14)).astype(np.uint8)
    b[rng.integers(0, one_in, size=(n, 14)) == 0] = 0x1A
    short = {"short": np.ones(n, bool), "long": np.zeros(n, bool), "alternate": np.arange(n) % 2 == 0,
             "random": rng.integers(0, 2, size=n) == 0}[mix]
    df = np.where(short, rng.choice(np.array(SHORT_DFS), n), rng.choice(np.array(LONG_DFS), n))
    b[:, 0] = df << 3 | (b[:, 0] & 7)
    b[short, 7:] = 0
    fr["bytes"], fr["fixed_bit"] = b, 0xFF
    lv = np.zeros(n, dtype=LEVEL_DTYPE)
    top = np.where(short, 60, 116) * LM.FULL_SCALE[sample_type]
    pool = rng.random(300) ** 2                       # 300 distinct loudnesses: the model's search runs once for each
    lv["signal_sum"] = (pool[rng.integers(0, 300, size=n)] * top).astype(np.uint64)
    lv["noise_sum"] = rng.integers(0, 1000, size=n)
    valid = rng.integers(0, 16, size=n) != 0
    lv["flags"] = np.where(valid, np.where(short, LM.VALID | LM.SHORT, LM.VALID), 0)
    return fr, lv


def is_short(frames):
    return (frames["bytes"][:, 0] >> 3) < 16


HOT_BIAS = 0x1A1A1A1A1A1A - 6 * 1000     # with offset 1000 the timestamp is 1A1A1A1A1A1A


def hot_short_frame(sample_type=I8):
    """(frames, levels, tick_bias): the short frame whose 14 payload bytes are all 0x1A, 30 bytes of Beast.  Its DF is 3
    (0x1A >> 3); the record is a SHORT one whose byte, scaled by 60, is 26."""
    fr = np.zeros(1, dtype=FRAME_DTYPE)
    fr["offset"], fr["fixed_bit"] = 1000, 0xFF
    fr["bytes"][0, :7] = 0x1A
    fr["bytes"][0, 7:] = 0x1A                 # never looked at: no escape may come from here
    lv = np.zeros(1, dtype=LEVEL_DTYPE)
    total = -(-(51 ** 2 * 60 * LM.FULL_SCALE[sample_type]) // (4 * 255 * 255))    # the smallest sum whose byte is 26
    lv["signal_sum"], lv["flags"] = total, LM.VALID | LM.SHORT
    assert LM.signal_byte(lv[0], sample_type) == 26 and LM.signal_byte(lv[0], sample_type, short_flag=False) != 26
    return fr, lv, HOT_BIAS


def wire_in_levels(signal, sample_type=I8):
    """wire input's records for these signal bytes: the smallest sum whose byte is s by 116, VALID, no SHORT"""
    lv = np.zeros(len(signal), dtype=LEVEL_DTYPE)
    for i, s in enumerate(signal):
        if s:
            lv[i]["signal_sum"], lv[i]["flags"] = smallest_sum_for(int(s), sample_type), 1
    return lv
