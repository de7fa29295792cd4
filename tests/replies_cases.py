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


# ---- the text only the device compiles -------------------------------------------------------------------------------
# Cases for what adsb_replies.hip has and the mirror has not: several candidates and several kept frames in one thread's
# run (one bitmap word), the sample-by-sample load of a ragged end, the last examined offset, the order in which
# workgroups take tiles, more channels than a workgroup has threads, every offset of a tile, and the capacity inside a
# word.  They are kept out of all_cases (its parametrised ids stay) and are built on demand, by name: the names need
# no building.  Every buffer ends in TAIL full-scale samples behind the last channel, as the gaps between channels
# hold: a read past a channel's end changes a result and stays inside the buffer.
TAIL = 256
AMPS = (120, 40, 12)                      # a group's members, each wholly weaker than the one before (I component)
_BUILT, _MODELS, _SHARED = {}, {}, {}


def run(dtype):
    """offsets per thread of the scan: one word of a tile's bitmap"""
    return tile(dtype) // 256


def stage(dtype, n, n_channels=1, stride=None, seed=None):
    """n_channels channels of n samples, zeros or (seed) low noise, stride apart; the gaps and TAIL samples behind the
    last channel are full-scale -> (the flat buffer, a view per channel)"""
    stride = n if stride is None else stride
    buf = np.full(((n_channels - 1) * stride + n + TAIL, 2), np.iinfo(dtype).min, dtype=dtype)
    views = []
    for c in range(n_channels):
        views.append(buf[c * stride:c * stride + n])
        views[c][:] = 0 if seed is None else M.noise(n, dtype, seed + c, LOW)
    return buf, views


def up8(n):
    return (n + 7) & ~7


def plant_preamble(iq, at, amp=100):
    """the four pulses of a preamble and nothing else"""
    for s in M.PULSES:
        iq[at + s] = (amp, 0)


def plant_group(iq, at, k, members):
    """`members` bare preambles k samples apart (10 <= k), the weaker written first and the stronger over them: on a zero
    background every one passes the strict test, reads its DF from its successor's pulses and is an address/parity
    candidate -> the members' offsets"""
    for m in reversed(range(members)):
        plant_preamble(iq, at + m * k, AMPS[m])
    return [at + m * k for m in range(members)]


def render_all(iq, msgs, offsets, pulse=(100, 0)):
    """M.render for many messages at once"""
    where = np.array([s for msg, at in zip(msgs, offsets) for s in M.pulse_positions(msg, at)], dtype=np.int64)
    iq[where[where < len(iq)]] = pulse
    return iq


def _shared(key, make):
    if key not in _SHARED:
        _SHARED[key] = make()
    return _SHARED[key]


# a. crowded runs
def _crowded(dt):
    """groups of two or three kept frames in one run: in the middle of a tile, pairs 10 and 12 apart, in the last run of
    waves 0, 1 and 2, two in one wave, in the last run of a tile with the last member at the tile's last offset (its
    long frames' halo is the next tile, which has groups of its own inside those frames), and at a tile's start"""
    T, R = tile(dt), run(dt)
    m3 = 3 if R == 32 else 2                 # members 14 apart that one run holds
    end = R - 1 - 14 * (m3 - 1)              # a group's first place when its last member is the run's last offset
    plan = [(0, 100, 0, 14, m3), (0, 40, 5, 10, 2), (0, 45, 3, 12, 2), (0, 63, end, 14, m3), (0, 127, end, 14, m3),
            (0, 191, end, 14, m3), (1, 70, 0, 14, m3), (1, 75, 2, 10, 2), (1, 255, end, 14, m3), (2, 32 // R, 0, 14, m3),
            (2, 96 // R, 0, 12, 2)]
    n = 3 * T + 777
    buf, views = stage(dt, n)
    groups = [plant_group(views[0], t * T + thread * R + place, k, m) for t, thread, place, k, m in plan]
    assert all(len({o // R for o in g}) == 1 for g in groups)
    c = case("crowded runs", buf, 1, n, n, [(0, o) for g in groups for o in g])
    c["groups"] = groups
    return c


def crowded_members(dtype):
    """per planted group of "crowded runs": (offset, the syndrome the model reports for it, None if it is not kept)"""
    dt = np.dtype(dtype)
    frames = device_text_model(dt, "crowded runs")[0]
    syn = {int(f["offset"]): MM.syndrome(bytes(f["bytes"])) for f in frames}
    return [[(o, syn.get(o)) for o in g] for g in device_text_case(dt, "crowded runs")["groups"]]


WHICH = {"first": 0, "middle": 1, "last": -1}


def _which(dt):
    return ("first", "middle", "last") if run(dt) == 32 else ("first", "last")


def _chosen(dt, which):
    """the syndromes of the chosen member of every group whose members differ in theirs (the pairs of two DF0 of zeros do
    not; the middle one: of groups of three), and of all the other members"""
    chosen, others = set(), set()
    for g in crowded_members(dt):
        distinct = len({s for _, s in g}) == len(g) and not (which == "middle" and len(g) < 3)
        pick = g[WHICH[which]] if distinct else None
        for member in g:
            if member[1] is not None:
                (chosen if member is pick else others).add(member[1])
    return chosen, others


def _crowded_known(dt, which, kept):
    base = device_text_case(dt, "crowded runs")
    chosen, others = _chosen(dt, which)
    known = np.array(sorted(chosen if kept else others - chosen), dtype=np.uint32)
    inside = set(known.tolist())
    members = [m for g in crowded_members(dt) for m in g]
    c = case(_known_name(which, kept), base["iq"], 1, base["n_samples"], base["n_samples"],
             [(0, o) for o, s in members if s in inside], [(0, o) for o, s in members if s not in inside], known=known, ap="known")
    c["groups"], c["which"], c["kept"] = base["groups"], which, kept
    return c


def _known_name(which, kept):
    return f"crowded runs, {'only' if kept else 'all but'} the {which} members known"


def crowded_cuts(dtype):
    """name -> max_frames: the whole list, one less, after the first and the second member of the word in the middle of
    tile 0, after the first member of the word that ends tile 1, and on the first frame of tile 1"""
    dt = np.dtype(dtype)
    T = tile(dt)
    offsets = device_text_model(dt, "crowded runs")[0]["offset"].tolist()
    groups = device_text_case(dt, "crowded runs")["groups"]
    return {"the total": len(offsets), "the total less one": len(offsets) - 1,
            "after a word's first member": offsets.index(groups[0][0]) + 1,
            "after a word's second member": offsets.index(groups[0][0]) + 2,
            "inside a tile's last word": offsets.index(groups[8][0]) + 1,
            "on a tile's first frame": next(k for k, o in enumerate(offsets) if o >= T) + 1}


CUTS = ("the total", "the total less one", "after a word's first member", "after a word's second member",
        "inside a tile's last word", "on a tile's first frame")


def _crowded_cut(dt, cut):
    base = device_text_case(dt, "crowded runs")
    return case(f"crowded runs, the capacity {cut}", base["iq"], 1, base["n_samples"], base["n_samples"],
                max_frames=crowded_cuts(dt)[cut])


# b. ragged ends
RAGGED_KINDS = (11, 18, 4, 20)


def ragged_lengths(dtype):
    T = tile(dtype)
    return [2 * T + 496 + r for r in range(1, 8)] if np.dtype(dtype) == np.int8 else [2 * T + 500 + r for r in range(1, 4)]


def _ragged(dt, n, past):
    """one frame per channel at the last offset it fits (past = 0) or one behind it; DF11 and DF18 are kept by their last
    24 bits, DF4 and DF20 by theirs under the known filter: the scan decides from the powers it loaded sample by sample,
    whatever the list is sliced from afterwards"""
    r = n % 8
    stride = up8(n)
    buf, views = stage(dt, n, len(RAGGED_KINDS), stride, seed=400 + 10 * r)
    where, known = [], []
    for c, df in enumerate(RAGGED_KINDS):
        at = n - span(df) + past
        k = 5 * r + 3 * c + 1
        if c % 2:                          # DF18 and DF20 end in 1111: a first half that reads its neighbour's power is a 0
            k = next(j for j in range(k, k + 4096) if message(df, AA + 16 * r + c, j)[-1] & 0xF == 0xF)
        M.render(views[c], message(df, AA + 16 * r + c, k), at)
        where.append((c, at))
        if df in M.ADDRESS_PARITY:
            known.append(AA + 16 * r + c)
    return case(_ragged_name(n, past, dt), buf, len(RAGGED_KINDS), n, stride, () if past else where, where if past else (),
                known=np.array(sorted(known), dtype=np.uint32), ap="known")


def _ragged_name(n, past, dt):
    return f"a ragged end, n = 2T+{n - 2 * tile(dt)}, the frames at the last offset" + (" + 1" if past else "")


SHORT_LENGTHS = (26, 27, span(11), span(11) + 1, span(20), span(20) + 1)


def _short(dt, n):
    """three touching channels of n samples with a DF11, a DF20 and a DF4 at the last offset each fits, or, if it does
    not fit, at the last examined offset (counted, not kept)"""
    stride = up8(n)
    buf, views = stage(dt, n, 3, stride)
    present, absent = [], []
    for c, df in enumerate((11, 20, 4)):
        fits = n >= span(df)
        at = n - span(df) if fits else n - 26
        M.render(views[c], message(df, AA + c, n + c), at)
        (present if fits else absent).append((c, at))
    return case(f"three channels of {n} samples", buf, 3, n, stride, present, absent)


# c. the window rule
def window_lengths(dtype):
    T = tile(dtype)
    return {"26": 26, "27": 27, "T+25": T + 25, "T+26": T + 26, "T+29": T + 29, "2T+28": 2 * T + 28}


def _window(dt, label, back, n_channels):
    """a bare preamble at n - back in every channel: n - 26 is the last examined offset (counted, no frame fits), n - 25
    is not examined"""
    n = window_lengths(dt)[label]
    stride = up8(n)
    buf, views = stage(dt, n, n_channels, stride)
    for v in views:
        plant_preamble(v, n - back)
    c = case(_window_name(label, back, n_channels), buf, n_channels, n, stride, (), [(ch, n - back) for ch in range(n_channels)])
    c["n_preamble"] = n_channels if back == 26 else 0
    return c


def _window_name(label, back, n_channels):
    return f"a bare preamble at n-{back}, n = {label}, {n_channels} channel" + ("s" if n_channels > 1 else "")


# d. every tile
def _tiles(dt, n_channels, tiles):
    """one short frame in every tile of every channel, at a place of its own; the last tile examines T offsets"""
    T = tile(dt)
    n = tiles * T + 25
    stride = up8(n)
    buf, views = stage(dt, n, n_channels, stride, seed=500 + tiles)
    present = []
    for ch in range(n_channels):
        for i in range(tiles):
            k = i + tiles * ch
            at = i * T + (37 + 1201 * k) % (T - 128)
            M.render(views[ch], message((11, 4, 5, 0)[k % 4], AA + k, k), at)
            present.append((ch, at))
    c = case(_tiles_name(n_channels, tiles), buf, n_channels, n, stride, present)
    c["zeros_first"] = True                # the GPU tier runs zeros of this length first: nothing stale stands in
    return c


def _tiles_name(n_channels, tiles):
    return f"a frame in every tile, {n_channels} x {tiles}"


TILES = [(1, k) for k in range(1, 18)] + [(3, 5), (8, 3)]


# e. many short channels
MANY = 300


def _many_136(dt):
    """300 touching channels of 136 samples, a short frame in channel c at offset c % 17: up to 8 it fits, from 9 on it runs
    into the next channel (absent, counted as a preamble).  The eight samples that channel 16, 33, ... spill are in the
    gaps of the next channel's preamble at offset 0, which therefore is none."""
    n = 136
    buf, _ = stage(dt, n, MANY, n)
    present, absent = [], []
    for c in range(MANY):
        M.render(buf, message((11, 4, 5, 0)[c % 4], AA + c, c), c * n + c % 17)
        fits = c % 17 <= 8 and not (c % 17 == 0 and c > 0)
        (present if fits else absent).append((c, c % 17))
    c = case("300 channels of 136 samples", buf, MANY, n, n, present, absent)
    c["n_preamble"] = MANY - len([k for k in range(1, MANY) if k % 17 == 0])
    return c


def _many_26(dt):
    """300 channels of 26 samples: one examined offset per tile; a bare preamble in two channels of three"""
    buf, views = stage(dt, 26, MANY, 32)
    marked = [c for c in range(MANY) if c % 3]
    for c in marked:
        plant_preamble(views[c], 0)
    c = case("300 channels of 26 samples", buf, MANY, 26, 32, (), [(ch, 0) for ch in marked])
    c["n_preamble"] = len(marked)
    return c


# f. every in-tile offset
OFFSETS = {"short": (129, (11, 4, 5, 0)), "long": (241, (16, 18, 20, 21))}


def _offsets_buffer(dt, kind):
    def make():
        T = tile(dt)
        step, dfs = OFFSETS[kind]
        n = step * T
        buf, views = stage(dt, n, seed=600)
        offsets = [k * step for k in range(T)]
        render_all(views[0], [message(dfs[k % 4], AA + k, k) for k in range(T)], offsets)
        return buf, n, offsets
    return _shared(("offsets", dt.name, kind), make)


def _offsets(dt, kind, filtered):
    """T frames whose starts take every residue mod T once (the step is odd); with the filter, the even-indexed addresses
    are known: DF11 and DF18 stay, every second address/parity frame goes"""
    buf, n, offsets = _offsets_buffer(dt, kind)
    dfs = OFFSETS[kind][1]
    if not filtered:
        return case(_offsets_name(kind, filtered), buf, 1, n, n, [(0, o) for o in offsets])
    stays = [dfs[k % 4] in (11, 18) or k % 2 == 0 for k in range(len(offsets))]
    return case(_offsets_name(kind, filtered), buf, 1, n, n, [(0, o) for o, s in zip(offsets, stays) if s],
                [(0, o) for o, s in zip(offsets, stays) if not s],
                known=np.arange(AA, AA + len(offsets), 2, dtype=np.uint32), ap="known")


def _offsets_name(kind, filtered):
    return f"every in-tile offset, {kind} frames" + (", the even addresses known" if filtered else "")


FAMILIES = ("crowded", "ragged", "window", "tiles", "channels", "offsets")


def _plan(dtype):
    """(family, name, builder) of every case, in order; nothing is built here"""
    dt = np.dtype(dtype)
    plan = [("crowded", "crowded runs", lambda: _crowded(dt))]
    for which in _which(dt):
        for kept in (True, False):
            plan.append(("crowded", _known_name(which, kept), lambda which=which, kept=kept: _crowded_known(dt, which, kept)))
    for cut in CUTS:
        plan.append(("crowded", f"crowded runs, the capacity {cut}", lambda cut=cut: _crowded_cut(dt, cut)))
    for n in ragged_lengths(dt):
        for past in (0, 1):
            plan.append(("ragged", _ragged_name(n, past, dt), lambda n=n, past=past: _ragged(dt, n, past)))
    for n in SHORT_LENGTHS:
        plan.append(("ragged", f"three channels of {n} samples", lambda n=n: _short(dt, n)))
    for n_channels in (1, 3):
        for label in window_lengths(dt):
            for back in (26, 25):
                plan.append(("window", _window_name(label, back, n_channels),
                             lambda label=label, back=back, n_channels=n_channels: _window(dt, label, back, n_channels)))
    for n_channels, tiles in TILES:
        plan.append(("tiles", _tiles_name(n_channels, tiles), lambda n_channels=n_channels, tiles=tiles: _tiles(dt, n_channels, tiles)))
    plan.append(("channels", "300 channels of 136 samples", lambda: _many_136(dt)))
    plan.append(("channels", "300 channels of 26 samples", lambda: _many_26(dt)))
    for kind in OFFSETS:
        for filtered in (False, True):
            plan.append(("offsets", _offsets_name(kind, filtered), lambda kind=kind, filtered=filtered: _offsets(dt, kind, filtered)))
    return plan


def device_text_names(dtype, families=FAMILIES):
    return [name for family, name, _ in _plan(dtype) if family in families]


def device_text_case(dtype, name):
    """the case of that name, built once; the tests leave it unchanged"""
    key = (np.dtype(dtype).name, name)
    if key not in _BUILT:
        made = next(make for _, n, make in _plan(dtype) if n == name)()
        assert made["name"] == name
        _BUILT[key] = made
    return _BUILT[key]


def device_text_cases(dtype, families=FAMILIES):
    return [device_text_case(dtype, name) for name in device_text_names(dtype, families)]


def device_text_model(dtype, name):
    """the model's answer to that case, computed once"""
    key = (np.dtype(dtype).name, name)
    if key not in _MODELS:
        _MODELS[key] = run_model(device_text_case(dtype, name))
    return _MODELS[key]


# g. the merge with many channels
def merge_many_channels():
    """(name, a, counts_a, b, counts_b): 5000 channels with 0 to 3 frames in either list, offsets from a small range (ties
    inside a list and between the lists), runs of channels empty in both lists at the start, in the middle and at the
    end, and one channel with 600 frames in list a and 450 in list b"""
    def make():
        rng = np.random.default_rng(31)
        n_channels, crowd = 5000, 1234
        counts = rng.choice(np.array([0, 0, 0, 1, 2, 3]), size=(2, n_channels))
        for lo, hi in ((0, 40), (2000, 2300), (n_channels - 55, n_channels)):
            counts[:, lo:hi] = 0
        counts[0, crowd], counts[1, crowd] = 600, 450
        lists = []
        for which in range(2):
            offsets = np.concatenate([np.sort(rng.integers(0, 400 if c == crowd else 6, k)) for c, k in enumerate(counts[which])])
            msgs = [message(11, AA + 100000 * which + k, k) for k in range(len(offsets))]
            lists.append(MM.frame_list(msgs, offsets=offsets.astype(np.uint64)))
        return ("5000 channels", lists[0], counts[0].tolist(), lists[1], counts[1].tolist())
    return _shared("merge", make)
