"""The cases of the replies scan's tests: sample buffers a few tiles long with what the scan must find in them.  Every
case is a dict: name, iq (flat [samples, 2] int8 / int16), n_channels, n_samples, channel_stride, kw (known, ap,
max_frames, first_sample), present / absent: (channel, offset) pairs that must / must not be in the list.  The CPU tier
runs them through the mirror and the model, the GPU tier through the device as well; T is the scan's tile length for
the sample type (adsb_debug_replies_geometry), which needs no device to ask."""
import ctypes as C

import numpy as np

from air_rs_amd import _lib as L
from tests import modes_model as MM
from tests import replies_model as M

ACCEPTED = (11, 18, 0, 4, 5, 16, 20, 21)
LOW = 2                                   # the noise under planted frames: I, Q in [-2, 2], p <= 8
AA = 0x4B1A2C


def tile(dtype):
    a, b = C.c_uint32(), C.c_uint32()
    assert L.load().adsb_debug_replies_geometry(C.byref(a), C.byref(b)) == 0
    return a.value if np.dtype(dtype) == np.int8 else b.value


def message(df, address=AA, k=0):
    """a valid message of an accepted (or any other) DF"""
    if df == 11:
        return MM.all_call(address, iid=k % 128)
    if df in (17, 18):
        return MM.squitter(address, df=df, ca=0 if df == 18 else 5, me=bytes([0x58, k & 0xFF, 3, 4, 5, 6, 7]))
    if df in M.ADDRESS_PARITY:
        return MM.reply(df, address, low3=k % 6, b1=(k * 8) & 0xFF, field=0x1838 ^ (k & 0xFFF), rest=bytes([0x20, 1, 2, 3, 4, 5, k & 0xFF]))
    if df >= 16:                          # formats the scan never keeps
        return MM.overlay(bytes([df << 3]) + bytes(range(1, 11)), 0)
    return MM.overlay(bytes([df << 3, 1, 2, 3]), 0)


def bits_len(df):
    return 56 if df < 16 else 112


def span(df):
    return 16 + 2 * bits_len(df)


def case(name, iq, n_channels=1, n_samples=None, channel_stride=None, present=(), absent=(), **kw):
    iq = np.ascontiguousarray(iq)
    n_samples = len(iq) // n_channels if n_samples is None else n_samples
    return dict(name=name, iq=iq, n_channels=n_channels, n_samples=n_samples,
                channel_stride=n_samples if channel_stride is None else channel_stride, present=list(present),
                absent=list(absent), kw=kw)


def channels(dtype, n, stride, n_channels, seed):
    """n_channels channels of low noise, stride apart; the gaps hold full-scale samples (a wrong stride shows)"""
    lo = np.iinfo(dtype).min
    buf = np.full(((n_channels - 1) * stride + n, 2), lo, dtype=dtype)
    views = []
    for c in range(n_channels):
        buf[c * stride:c * stride + n] = M.noise(n, dtype, seed + c, LOW)
        views.append(buf[c * stride:c * stride + n])
    return buf, views


def edges(dtype):
    """one frame of every accepted DF, one DF per channel, at offsets 0, T-1, T, T+1, the last that can be emitted and one
    past it (absent, and cut by the channel's end); two tiles and a ragged third"""
    T = tile(dtype)
    n, out = 2 * T + 504, []
    stride = n + 8
    for where in ("0", "T-1", "T", "T+1", "last", "last+1"):
        buf, views = channels(dtype, n, stride, len(ACCEPTED), 100)
        present, absent = [], []
        for c, df in enumerate(ACCEPTED):
            at = {"0": 0, "T-1": T - 1, "T": T, "T+1": T + 1, "last": n - span(df), "last+1": n - span(df) + 1}[where]
            M.render(views[c], message(df, AA + c, c), at)
            (absent if where == "last+1" else present).append((c, at))
        out.append(case(f"edges at {where}", buf, len(ACCEPTED), n, stride, present, absent))
    return out


def channel_edge(dtype):
    """a frame that starts in channel 0 and ends in channel 1 (stride = n_samples: the channels touch) is absent; the same
    frame wholly inside channel 1 is present; one channel and three, stride above n_samples, a ragged last tile"""
    T = tile(dtype)
    n = T + 1000                                     # (a multiple of 8)
    buf, views = channels(dtype, n, n, 3, 200)
    M.render(buf, message(20), n - 100)              # across the edge, in the flat buffer
    M.render(views[1], message(4), 300)
    M.render(views[2], message(11), n - span(11))
    out = [case("a window across a channel edge", buf, 3, n, n, [(1, 300), (2, n - span(11))], [(0, n - 100)])]
    n = 2 * T + 776
    buf, views = channels(dtype, n, n + 16, 3, 210)
    present = []
    for c, (df, at) in enumerate(((0, 5), (21, T - 3), (16, n - span(16)))):
        M.render(views[c], message(df, AA + c, c), at)
        present.append((c, at))
    out.append(case("three channels, a stride above n_samples", buf, 3, n, n + 16, present, first_sample=10**12 + 7))
    one = np.ascontiguousarray(views[1])
    out.append(case("one channel, a ragged last tile", one, 1, n, None, [(0, T - 3)]))
    return out


def every_lane(dtype):
    """short frames every 131 samples over four tiles: every place a run of offsets has"""
    T = tile(dtype)
    n = 4 * T + 131
    iq = M.noise(n, dtype, 300, LOW)
    present = []
    for k, at in enumerate(range(0, n - span(11), 131)):
        df = (11, 4, 5, 0)[k % 4]
        M.render(iq, message(df, AA + k, k), at)
        present.append((0, at))
    return [case("short frames every 131 samples", iq, present=present)]


def dense(dtype):
    """DF11 back to back every 128 samples through two whole tiles; the same with the capacity inside the second tile"""
    T = tile(dtype)
    n = 2 * T + 128
    iq = np.zeros((n, 2), dtype=dtype)
    present = []
    for k, at in enumerate(range(0, 2 * T, 128)):
        M.render(iq, message(11, AA + k, k), at)
        present.append((0, at))
    cut = T // 128 + 5
    return [case("dense DF11", iq, present=present),
            case("dense DF11, the capacity inside a tile", iq, max_frames=cut)]   # (the tests hold it to the whole list's head)


def ties(dtype):
    """the strict preamble, the bit tie, the largest CS16 power, constant and zero buffers"""
    T = tile(dtype)
    n = T + 600
    out = []
    for name, gap_q, found in (("a preamble whose weakest pulse equals its strongest gap", 0, False),
                               ("... and one unit above it", 1, True)):
        iq = np.zeros((n, 2), dtype=dtype)
        M.render(iq, message(4), 40, pulse=(50, gap_q))     # p = 2500 (+1)
        iq[40 + 5] = (50, 0)                                 # a gap sample at 2500
        out.append(case(name, iq, present=[(0, 40)] if found else (), absent=() if found else [(0, 40)]))
    msg = message(5)
    bits = np.unpackbits(np.frombuffer(msg, dtype=np.uint8))
    k = int(np.nonzero(bits[8:] == 0)[0][0]) + 8             # a 0 bit behind the DF: its pulse is in the second half
    iq = np.zeros((n, 2), dtype=dtype)
    M.render(iq, msg, 77)
    iq[77 + 16 + 2 * k] = iq[77 + 17 + 2 * k]               # both halves alike: reads 0, the frame stays valid
    out.append(case("a bit tie reads 0", iq, present=[(0, 77)]))
    if np.dtype(dtype) == np.int16:
        iq = np.zeros((n, 2), dtype=dtype)
        M.render(iq, message(20), T - 9, pulse=(-32768, -32768))
        M.render(iq, message(11), 3, pulse=(-32768, -32768))
        out.append(case("CS16 pulses at (-32768, -32768)", iq, present=[(0, 3), (0, T - 9)]))
    else:
        out.append(case("an i8 buffer of constants", np.full((n, 2), -128, dtype=dtype)))
        out.append(case("an i8 buffer of zeros", np.zeros((n, 2), dtype=dtype)))
    return out


def decisions(dtype):
    """what DF and syndrome decide, and the known filter with 0, 1 and 4096 addresses"""
    T = tile(dtype)
    n = T + 3000
    iq = np.zeros((n, 2), dtype=dtype)
    present, absent, at = [], [], 10
    plan = [(MM.all_call(AA, iid=0), True), (MM.all_call(AA, iid=1), True), (MM.all_call(AA, iid=127), True),
            (MM.overlay(bytes([11 << 3 | 5]) + AA.to_bytes(3, "big"), 128), False),
            (message(18), True), (bytes([message(18)[0], message(18)[1] ^ 0x10]) + message(18)[2:], False),
            (message(17), False), (message(1), False), (message(19), False), (message(24), False)]
    for msg, keep in plan:
        M.render(iq, msg, at)
        (present if keep else absent).append((0, at))
        at += 300
    out = [case("DF and syndrome", iq, present=present, absent=absent)]
    rng = np.random.default_rng(5)
    drawn = np.unique(rng.integers(1, 0xFFFFFF, 6000, dtype=np.uint32))          # (ascending, distinct, neither end)
    table = np.sort(np.concatenate([rng.permutation(drawn)[:4094], np.array([0, 0xFFFFFF], dtype=np.uint32)]))
    assert len(table) == 4096 and table[0] == 0 and table[-1] == 0xFFFFFF and (np.diff(table.astype(np.int64)) > 0).all()
    middle = int(table[2000])
    members = set(table.tolist())
    outside = next(a for a in range(0x123456, 0x123556) if a not in members and a + 1 not in members)
    iq = np.zeros((n, 2), dtype=dtype)
    placed = []
    for k, (df, address) in enumerate(((4, 0), (20, 0xFFFFFF), (5, middle), (0, outside), (21, int(table[1])), (16, outside + 1))):
        M.render(iq, message(df, address, k), 20 + 300 * k)
        placed.append((20 + 300 * k, address))
    for name, known in (("no", np.zeros(0, dtype=np.uint32)), ("one", np.array([0xFFFFFF], dtype=np.uint32)),
                        ("its first", np.array([0], dtype=np.uint32)), ("4096", table)):
        inside = set(known.tolist())
        out.append(case(f"the known filter with {name} addresses", iq, present=[(0, o) for o, a in placed if a in inside],
                        absent=[(0, o) for o, a in placed if a not in inside], known=known, ap="known"))
    out.append(case("address/parity frames without the filter", iq, present=[(0, o) for o, _ in placed]))
    return out


def pure_noise(dtype):
    T = tile(dtype)
    n = 5 * T + 333 if np.dtype(dtype) == np.int8 else 10 * T + 333
    return [case("seeded noise", M.noise(n, dtype, 77, 127 if np.dtype(dtype) == np.int8 else 20000))]


def all_cases(dtype):
    out = []
    for make in (edges, channel_edge, every_lane, dense, ties, decisions, pure_noise):
        out += make(dtype)
    return out


def ids(dtype):
    return [c["name"] for c in all_cases(dtype)]


def run_model(c):
    return M.replies(c["iq"], c["n_channels"], c["n_samples"], c["channel_stride"], **c["kw"])


def check_expectations(c, frames, counts):
    """the case's own present / absent lists against a result (so that model, mirror and device cannot agree on nothing)"""
    first = c["kw"].get("first_sample", 0)
    at, have = 0, set()
    for ch, cnt in enumerate(counts):
        have |= {(ch, int(o) - first) for o in frames["offset"][at:at + int(cnt)]}
        at += int(cnt)
    assert at == len(frames)
    missing = [p for p in c["present"] if tuple(p) not in have]
    extra = [p for p in c["absent"] if tuple(p) in have]
    assert not missing and not extra, (c["name"], missing[:5], extra[:5])


# ---- merge -----------------------------------------------------------------------------------------------------------
def merge_cases():
    """(name, a, counts_a, b, counts_b): equal offsets, an empty channel, either list empty, many frames"""
    def fl(offsets, tag):
        fr = MM.frame_list([message(11, AA + tag + k, k) for k in range(len(offsets))], offsets=np.array(offsets, dtype=np.uint64))
        return fr
    rng = np.random.default_rng(9)
    big_a = np.sort(rng.integers(0, 5000, 700)).tolist() + np.sort(rng.integers(0, 5000, 300)).tolist()
    big_b = np.sort(rng.integers(0, 5000, 10)).tolist() + np.sort(rng.integers(0, 5000, 900)).tolist()
    return [("equal offsets", fl([5, 9, 9, 20], 0), [4], fl([1, 9, 20, 20, 30], 100), [5]),
            ("an empty channel", fl([3, 7, 2], 0), [2, 0, 1], fl([4, 1, 2, 3], 100), [1, 0, 3]),
            ("list a empty", fl([], 0), [0, 0], fl([4, 1], 100), [1, 1]),
            ("list b empty", fl([4, 1], 0), [1, 1], fl([], 100), [0, 0]),
            ("both empty", fl([], 0), [0], fl([], 100), [0]),
            ("many frames with ties", fl(big_a, 0), [700, 300], fl(big_b, 2000), [10, 900])]
