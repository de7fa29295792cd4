"""A real frame at every in-tile offset (tests/test_sweep_cases.py checks the builders on the CPU, tests/test_gpu_position_sweep.py
and tests/ab_cases.py run them on the device).

The scan kernels deal every offset of a tile to one lane, park the magnitudes in LDS as packed bytes or halfwords and slice 240
of them from an arbitrary LDS address.  The constant buffer reaches every in-tile offset and cannot see which sample a lane
reads: every magnitude is equal.  Here frame k sits at lead + stride * k, k = 0 .. tile - 1, with gcd(stride, tile) = 1: the
offsets mod tile are 0 .. tile - 1, each once, and every one of them carries a frame that is right only if exactly its own 240
samples were read.

  frames    frame k is its own valid DF17 frame (0x8D, ten bytes seeded by k, the oracle's CRC): two exchanged positions show as
            wrong bytes, not only as a wrong count.
  rotate    frame k carries what the unrotated sweep's frame k + rotate carries: bytes, class, level and flipped bit.
  classes   by (k + rotate) % 3: CLEAN (status 0); FLIP: data bit j flipped, j = 5 + ((k + rotate) // 3) % 83 (status 1, fixed_bit j, the
            clean bytes); TIE: every 0 bit is a tie of hi against hi -- the strict slicer reads 0, the gate passes on >=.
  levels    by ((k + rotate) // 3) % len(levels): (hi, lo, bg) as ROOTS.  Not by k: with six levels k % 6 would fix k % 3, and every level
            must meet every class.  A level whose tie frame the oracle itself does not return (tie_ok) keeps CLEAN in its place.
  samples   real (I, Q) pairs: each magnitude m is a seeded random representative with isqrt(I * I + Q * Q) == m, both signs,
            both components non-zero where m allows (i8: all 65 536 pairs enumerated; CS16: I drawn, Q solved for, checked with
            math.isqrt).  So both positions of the i8 scan's paired dots and CS16's correction step pass every in-tile offset.
  between   the lead, the gap behind every frame and the tail alternate 0 / bg, bg >= 1, to the buffer's last sample: a stretch
            of 240 equal samples would emit a frame per offset.  The alternation turns round 16 samples into
            every gap (see build).
  big       (CS16) one sample of root >= 31744 in a gap of every tile, outside every planted window: every tile takes the
            integer gate.
  shift     the first `shift` samples are dropped (whole tiles of background are put in front first where frame 0 would go
            with them): the offsets mod tile stay a bijection, and every frame meets another offset and another dword alignment.

compare() is the device tests' assertion: on a mismatch it names the first differing frames by tile and in-tile offset and the
set of in-tile offsets that are missing or wrong, as ranges -- a wrong lane, run or wave shows as a pattern."""
import math
import time
from collections import namedtuple

import numpy as np

from tests import survivor_cases as S
from tests.oracle_binding import FRAME_DTYPE

WINDOW = S.WINDOW
LEAD = 7         # samples in front of frame 0: offset 0 is not special
TAIL = 37        # ragged samples behind the last frame's window
GAP_TURN = 16    # samples of a gap before its alternation turns round (see build)
SEED = 1090
F16_LIMIT = 31744
CLEAN, FLIP, TIE = 0, 1, 2
CLASSES = ("clean", "flip", "tie")
FLIP_BITS = tuple(range(5, 88))
SLICE_TILES = 32  # the one-dispatch path takes at most 32 tiles + 240 samples

LEVELS_I8 = ((100, 0, 10), (41, 40, 40), (181, 180, 3), (1, 0, 1), (181, 0, 181), (60, 59, 1))
LEVELS_CS16 = ((100, 0, 10), (31743, 31742, 5), (20000, 19999, 19999), (1, 0, 1), (31743, 0, 31743))
LEVELS_CS16_BIG = LEVELS_CS16 + ((40000, 39999, 11),)
BIG_ROOT = 40000

Sweep = namedtuple("Sweep", "iq planted mag tile stride levels level_of class_of flip_of big_at")


# ---- frames -----------------------------------------------------------------------------------------------------------------
_FRAMES = []


def frames(oracle, n):
    """uint8 [n, 14]: frame k = 0x8D, ten bytes from a generator seeded by k, the oracle's CRC"""
    while len(_FRAMES) < n:
        k = len(_FRAMES)
        data = bytes([0x8D]) + bytes(np.random.default_rng([SEED, k]).integers(0, 256, size=10, dtype=np.uint8))
        crc = oracle.get_adsb_crc(data)
        _FRAMES.append(data + bytes([(crc >> 16) & 0xFF, (crc >> 8) & 0xFF, crc & 0xFF]))
    out = np.frombuffer(b"".join(_FRAMES[:n]), dtype=np.uint8).reshape(n, 14)
    assert len(set(_FRAMES[:n])) == n
    return out


# ---- representatives of a root ------------------------------------------------------------------------------------------------
_REPS = {}
REPS_PER_ROOT = 2048  # CS16 draws per root


def _ceil_sqrt(v):
    return 0 if v <= 0 else math.isqrt(v - 1) + 1


def _reps_i8():
    i, q = np.meshgrid(np.arange(-128, 128), np.arange(-128, 128), indexing="ij")
    i, q = i.ravel(), q.ravel()
    root = np.array([math.isqrt(int(n)) for n in range(2 * 128 * 128 + 1)])[i * i + q * q]
    table = {}
    for m in range(182):
        pick = root == m
        both = pick & (i != 0) & (q != 0)
        pick = both if both.any() else pick
        table[m] = np.stack([i[pick], q[pick]], axis=1).astype(np.int8)
    return table


def _reps_cs16(m):
    """REPS_PER_ROOT pairs of i16 with root m: |I| drawn, |Q| drawn among the values that keep I^2 + Q^2 in [m^2, (m + 1)^2 - 1],
    the two exchanged and signed from the seed"""
    rng = np.random.default_rng([SEED, m])
    lo, hi = m * m, (m + 1) * (m + 1) - 1
    a_min = max(1 if m else 0, _ceil_sqrt(lo - 32767 * 32767))
    a_max = min(m, 32767)
    out = np.empty((REPS_PER_ROOT, 2), dtype=np.int16)
    k = 0
    while k < REPS_PER_ROOT:
        a = int(rng.integers(a_min, a_max + 1))
        b_min, b_max = _ceil_sqrt(lo - a * a), min(math.isqrt(hi - a * a), 32767)
        if b_min == 0 and b_max >= 1:
            b_min = 1
        if b_min > b_max:
            continue
        b = int(rng.integers(b_min, b_max + 1))
        assert math.isqrt(a * a + b * b) == m, (m, a, b)
        if rng.integers(0, 2):
            a, b = b, a
        out[k] = (-a if rng.integers(0, 2) else a, -b if rng.integers(0, 2) else b)
        k += 1
    return out


def reps(dtype, m):
    """every (I, Q) this module may use for the root m, as an array [count, 2]"""
    key = (np.dtype(dtype).name, int(m))
    if key not in _REPS:
        if np.dtype(dtype) == np.int8:
            for r, tab in _reps_i8().items():
                _REPS[(key[0], r)] = tab
        else:
            _REPS[key] = _reps_cs16(int(m))
        tab = _REPS[key].astype(np.int64)
        n = tab[:, 0] * tab[:, 0] + tab[:, 1] * tab[:, 1]
        assert len(tab) and ((n >= m * m) & (n < (m + 1) * (m + 1))).all()
        assert m == 0 or (tab != 0).all()
    return _REPS[key]


def to_iq(mag, dtype, seed):
    """(I, Q) per magnitude: a representative of its root drawn from the seed"""
    roots = np.nonzero(np.bincount(mag))[0]
    inverse = np.zeros(int(roots[-1]) + 1, dtype=np.int64)
    inverse[roots] = np.arange(len(roots))
    inverse = inverse[mag]
    tables = [reps(dtype, int(m)) for m in roots]
    start = np.cumsum([0] + [len(t) for t in tables[:-1]])
    count = np.array([len(t) for t in tables])
    draw = np.random.default_rng([SEED, seed]).integers(0, 1 << 31, size=len(mag))
    return np.concatenate(tables)[start[inverse] + draw % count[inverse]]


# ---- the gate, in 32 bits (buffers of 17 M samples) -------------------------------------------------------------------------------
def gate(mag):
    """survivor_cases.gate without its int64 copies"""
    mag = np.asarray(mag, dtype=np.int32)
    n = len(mag) - WINDOW

    def fold(f, ks):
        out = mag[ks[0]:ks[0] + n].copy()
        for k in ks[1:]:
            f(out, mag[k:k + n], out=out)
        return out

    ok = fold(np.minimum, S.PRE_HIGHS) >= fold(np.maximum, S.PRE_LOWS)
    ok &= fold(np.minimum, S.DF_HIGHS) >= fold(np.maximum, S.DF_LOWS)
    return ok


def survivors_per_tile(mag, tile):
    g = gate(mag)
    return np.add.reduceat(g.astype(np.int32), np.arange(0, len(g), tile))


# ---- the builder ----------------------------------------------------------------------------------------------------------------
def images(frame_rows, hi, lo, cls, flip_bit):
    """int32 [n, 240]: the PPM image of every frame at its level and in its class"""
    n = len(frame_rows)
    bits = np.unpackbits(frame_rows, axis=1).astype(bool)                     # [n, 112], MSB first
    sent = bits.copy()
    rows = np.nonzero(cls == FLIP)[0]
    sent[rows, flip_bit[rows]] ^= True
    hi, lo = hi[:, None], lo[:, None]
    img = np.broadcast_to(lo, (n, WINDOW)).astype(np.int32)
    img[:, list(S.PRE_HIGHS)] = hi
    img[:, 16::2] = np.where(sent, hi, lo)
    img[:, 17::2] = np.where(sent, lo, hi)
    tie = (cls == TIE)[:, None] & ~sent
    img[:, 16::2] = np.where(tie, hi, img[:, 16::2])                           # a 0 bit of a TIE frame: hi against hi
    return img


_TIE_OK = {}


def tie_ok(oracle, dtype, level):
    """Does the oracle return a TIE frame at this level?  One frame in its own background, asked of the oracle itself; a level
    where it does not keeps CLEAN frames in the TIE places (build's `cls`)."""
    key = (np.dtype(dtype).name, tuple(level))
    if key not in _TIE_OK:
        hi, lo, bg = level
        f = frames(oracle, 3)[2:3]
        mag = np.zeros(300 + WINDOW + 300, dtype=np.int32)
        mag[1::2] = bg
        mag[300:300 + WINDOW] = images(f, np.array([hi]), np.array([lo]), np.array([TIE]), np.array([0]))[0]
        rc, got, found = oracle.process_buffer(to_iq(mag, dtype, 0), max_out=64)
        assert rc == 0
        _TIE_OK[key] = any(r["offset"] == 300 and r["status"] == 0 and r["bytes"].tobytes() == f[0].tobytes() for r in got)
    return _TIE_OK[key]


def build(oracle, sample_type, tile, stride, levels, rotate=0, shift=0, big_sample=False):
    """the whole record of one sweep (see the module's text); sample_type: np.int8 or np.int16"""
    dtype = np.dtype(sample_type)
    assert dtype in (np.int8, np.int16) and stride >= 257 and math.gcd(stride, tile) == 1
    assert shift >= 0
    assert all(hi > lo >= 0 and bg >= 1 for hi, lo, bg in levels)
    k = np.arange(tile)
    c = k + rotate                                                              # what frame k carries
    level_of = (c // 3) % len(levels)
    cls = c % 3
    no_tie = np.array([not tie_ok(oracle, dtype, lv) for lv in levels])
    cls[(cls == TIE) & no_tie[level_of]] = CLEAN
    flip_bit = FLIP_BITS[0] + (c // 3) % len(FLIP_BITS)
    lv = np.asarray(levels, dtype=np.int32)
    hi, lo, bg = lv[level_of, 0], lv[level_of, 1], lv[level_of, 2]

    front = 0 if shift < LEAD else tile * ((shift - LEAD) // tile + 1)          # whole tiles: the offsets mod tile stay
    at = front + LEAD + stride * k
    n = int(at[-1]) + WINDOW + TAIL
    # The gap behind frame k, counted from the frame's end (the lead belongs to frame 0): (0, bg) eight times, then (bg, 0) to
    # the next frame.  Not one alternation from the buffer's start: a window inside a TIE frame passes the gate wherever a
    # few of its bits are 0 (ties pass), an odd number of samples in it slices every pair of the frame as 0, an even number
    # in it slices the frame's own last bits, and (0, bg) pairs behind either made the all-zero frame of it, which is valid:
    # 16 000 extra frames at stride 1031.  So both alignments meet ones: 0 .. 0 1111111 0 .. 0 (a burst the CRC detects) and
    # bits 00000000 1 .. 1 (no run of trailing ones is a codeword: tests/test_sweep_cases.py).
    p = np.arange(n)
    region = np.clip((p - (front + LEAD)) // stride, 0, tile - 1)
    i = p - at[region] - WINDOW
    mag = np.where((i & 1) ^ (i >= GAP_TURN), bg[region], 0).astype(np.int32)
    fr = frames(oracle, rotate + tile)[rotate:]
    mag[at[:, None] + np.arange(WINDOW)] = images(fr, hi, lo, cls, flip_bit)

    big_at = []
    if big_sample:
        assert dtype == np.int16
        for t in range(-(-(n - shift - WINDOW) // tile)):
            first = t * tile + shift                                              # tile t of the shifted buffer, unshifted
            j = max(-(-(first - int(at[0]) - WINDOW) // stride), 0)               # the first gap that begins inside it
            q = int(at[0]) + stride * j + WINDOW + (stride - WINDOW) // 2
            if j >= tile - 1:
                q = int(at[-1]) + WINDOW + TAIL // 2                              # (no whole gap is left: the tail)
            assert first <= q < min(first + tile, n) and (at + WINDOW <= q).sum() == (at <= q).sum(), (t, q)
            mag[q] = BIG_ROOT
            big_at.append(q - shift)

    iq = to_iq(mag, dtype, tile * 4099 + stride)[shift:]
    mag = mag[shift:]
    planted = np.zeros(tile, dtype=FRAME_DTYPE)
    planted["offset"] = at - shift
    planted["bytes"] = fr
    planted["status"] = cls == FLIP
    planted["fixed_bit"] = np.where(cls == FLIP, flip_bit, 0xFF)
    for a in (iq, mag, planted):
        a.setflags(write=False)
    return Sweep(iq, planted, mag, tile, stride, tuple(levels), level_of, cls, flip_bit, tuple(big_at))


def sweep(oracle, sample_type, tile, stride, levels, rotate=0, shift=0, big_sample=False):
    """(the IQ buffer, the planted list as records of (offset, bytes, status, fixed_bit) by offset)"""
    s = build(oracle, sample_type, tile, stride, levels, rotate, shift, big_sample)
    return s.iq, s.planted


# ---- the buffers the device tests use --------------------------------------------------------------------------------------------
# name: (sample type, tile, stride, levels, rotate, shift, big_sample)
CASES = {
    "i8 dense": (np.int8, 16384, 257, LEVELS_I8, 0, 0, False),
    "i8 sparse": (np.int8, 16384, 1031, LEVELS_I8, 1, 0, False),
    "i8 dense shift 1": (np.int8, 16384, 257, LEVELS_I8, 2, 1, False),
    "i8 dense shift tile/2+5": (np.int8, 16384, 257, LEVELS_I8, 1, 16384 // 2 + 5, False),
    "cs16 dense": (np.int16, 8192, 257, LEVELS_CS16, 0, 0, False),
    "cs16 sparse": (np.int16, 8192, 521, LEVELS_CS16, 1, 0, False),
    "cs16 dense big": (np.int16, 8192, 257, LEVELS_CS16_BIG, 2, 0, True),
    "cs16 sparse big": (np.int16, 8192, 521, LEVELS_CS16_BIG, 0, 0, True),
    "i8 dense reg": (np.int8, 16128, 257, LEVELS_I8, 0, 0, False),             # the reg scan's tile (tests/ab_cases.py)
}
_BUILT = {}


def built(oracle, name):
    if name not in _BUILT:
        _BUILT[name] = build(oracle, *CASES[name])
    return _BUILT[name]


_REF = {}


def reference(oracle, name):
    """(the Sweep, the oracle's list over the whole buffer, the seconds it took): once per process"""
    if name not in _REF:
        s = built(oracle, name)
        t0 = time.perf_counter()
        rc, want, found = oracle.process_buffer(s.iq, max_out=4 * s.tile)
        assert rc == 0 and found == len(want), (name, rc, found)
        want.setflags(write=False)
        _REF[name] = (s, want, time.perf_counter() - t0)
    return _REF[name]


def slice_reference(oracle, name):
    """([(first sample, the slice's samples, the oracle's list over that slice)], the same of the last, ragged slice filled up to the
    others' length with an alternation of roots 0 and 1: for a launch whose channels have one length)"""
    if ("slices", name) not in _REF:
        s = built(oracle, name)
        out = []
        for a, n in slices(len(s.iq), s.tile):
            part = s.iq[a:a + n]
            rc, want, found = oracle.process_buffer(part, max_out=4 * s.tile)
            assert rc == 0 and found == len(want), (name, a, rc, found)
            out.append((a, part, want))
        a, part, _ = out[-1]
        full = SLICE_TILES * s.tile + WINDOW
        padded = np.empty((full, 2), dtype=s.iq.dtype)
        padded[:len(part)] = part
        padded[len(part):] = (np.arange(full - len(part)) & 1)[:, None]
        rc, want, found = oracle.process_buffer(padded, max_out=4 * s.tile)
        assert rc == 0 and found == len(want)
        _REF["slices", name] = (out, (a, padded, want))
    return _REF["slices", name]


def slices(n_samples, tile):
    """[(first sample, samples)] of the cuts at multiples of 32 tiles, each with its 240 samples of halo; the last one ragged"""
    step = SLICE_TILES * tile
    return [(a, min(step + WINDOW, n_samples - a)) for a in range(0, n_samples - WINDOW, step)]


def swap_at(iq, tile, residue):
    """a copy with samples residue and residue + 1 of every tile exchanged"""
    out = np.array(iq)
    a = np.arange(residue, len(iq) - 1, tile)
    out[a], out[a + 1] = iq[a + 1], iq[a]
    return out


# ---- the comparison and its report ------------------------------------------------------------------------------------------------
def ranges(values):
    """'3-7, 12, 4096-4159' of a set of integers"""
    v = np.unique(np.asarray(list(values), dtype=np.int64))
    if not len(v):
        return "none"
    cut = np.nonzero(np.diff(v) > 1)[0]
    first, last = np.r_[v[:1], v[cut + 1]], np.r_[v[cut], v[-1:]]
    return ", ".join(str(a) if a == b else f"{a}-{b}" for a, b in zip(first.tolist(), last.tolist()))


def _text(r, tile):
    return (f"tile {int(r['offset']) // tile} + {int(r['offset']) % tile}: {r['bytes'].tobytes().hex()} status {int(r['status'])} "
            f"fixed_bit {int(r['fixed_bit'])}")


def differences(got, want, tile, limit=4):
    """None where the lists are equal, else the report"""
    if len(got) == len(want) and (got == want).all():
        return None
    key = lambda a: {int(r["offset"]): r for r in a}
    g, w = key(got), key(want)
    same = lambda a, b: a.tobytes() == b.tobytes()
    missing = sorted(o for o in w if o not in g)
    extra = sorted(o for o in g if o not in w)
    wrong = sorted(o for o in w if o in g and not same(g[o], w[o]))
    lines = [f"{len(got)} frames, the oracle has {len(want)}: {len(missing)} missing, {len(wrong)} wrong, {len(extra)} extra"]
    if len(g) != len(got) or (np.diff(got["offset"].astype(np.int64)) <= 0).any():
        lines.append("the list's offsets do not ascend strictly")
    for name, offs in (("missing", missing), ("wrong", wrong), ("extra", extra)):
        for o in offs[:limit]:
            lines.append(f"  {name}  " + (_text(g[o], tile) + "  for  " + _text(w[o], tile) if name == "wrong" else
                                        _text((g if name == "extra" else w)[o], tile)))
        lines.append(f"  in-tile offsets {name}: " + ranges(o % tile for o in offs))
    lines.append("  tiles concerned: " + ranges(o // tile for o in missing + wrong + extra))
    return "\n".join(lines)


def compare(got, want, tile, what=""):
    text = differences(got, want, tile)
    assert text is None, f"{what}: {text}"
