"""Hand-built CS16 buffers that decide the CS16 scan's gate and slicer on real (I, Q) samples (tests/test_cs16_cases.py checks
the builders on the CPU, tests/test_gpu_cs16_gate.py runs them on the device).

survivor_cases.py builds MAGNITUDES as I = magnitude, Q = 0: perfect squares only.  Here a magnitude m is carried by a
REPRESENTATIVE of its root class [m^2, (m + 1)^2 - 1]: rep(m, "min") is the smallest I^2 + Q^2 of the class an i16 pair can reach,
rep(m, "max") the largest.  The reference orders floor(sqrt(I^2 + Q^2)) (utils.rs:46-52), so the two tie: a tie passes the gate
(>=) and slices as 0 (strict >).  A scan that orders I^2 + Q^2, or a rounded root, or takes the wrong one of the CS16 scan's two
gates, decides some window here differently.

The launch returns frames, not survivors, so every planted window is a whole valid DF17 frame whose sliced bits do not depend
on the samples that are moved: a window the device lets through against the reference comes back as a frame, one it rejects
against the reference goes missing.

A Window is 240 model magnitudes (the roots), its 240 (I, Q) samples, the frame it carries and the reference's verdict; a Buffer
is background + planted windows, as magnitudes (the model) and as samples (what the oracle and the device are given)."""
import math
from functools import lru_cache

import numpy as np

from tests import survivor_cases as S
from tests.oracle_binding import FRAME_DTYPE

TILE = 8192          # offsets per CS16 tile
HALO = 256           # samples a tile loads beyond its own (the ninth sweep, wave 0 alone)
F16_LIMIT = 31744    # 0x7C00: magnitudes below it are ordered non-negative finite f16 bit patterns
TOP = 46340          # floor(sqrt(2^31))
SMALL_TILES = 31     # full tiles per buffer: with the ragged one after them a launch still takes the one-dispatch path
SEED = 1090
CORNERS = ((32767, 32767), (32766, -32768), (32767, -32768), (-32768, -32768))


# ---- representatives of a root class --------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def class_ends(m):
    """((n, a, b) of the smallest reachable n = a^2 + b^2 with isqrt(n) == m, the same of the largest); a, b in 0..32768"""
    lo, hi = m * m, (m + 1) * (m + 1) - 1
    least = most = None
    # (some order of every pair has a >= b, so a^2 >= n / 2 >= lo / 2)
    for a in range(math.isqrt(lo // 2), min(math.isqrt(hi), 32768) + 1):
        rest = lo - a * a
        b = 0 if rest <= 0 else math.isqrt(rest - 1) + 1  # the least b with a^2 + b^2 >= lo
        n = a * a + b * b
        if b <= 32768 and n <= hi and (least is None or n < least[0]):
            least = (n, a, b)
        b = min(math.isqrt(hi - a * a), 32768)            # the greatest b with a^2 + b^2 <= hi
        n = a * a + b * b
        if n >= lo and (most is None or n > most[0]):
            most = (n, a, b)
    assert least is not None and most is not None and math.isqrt(least[0]) == m == math.isqrt(most[0]), m
    return least, most


def rep(m, which, seed=0):
    """an (I, Q) pair of i16 whose root is m: the class's smallest ("min") or largest ("max") I^2 + Q^2, signs from the seed
    (32768 exists as -32768 only)"""
    _, a, b = class_ends(m)[0 if which == "min" else 1]
    sa, sb = np.random.default_rng([SEED, seed, m, which == "max"]).integers(0, 2, size=2)
    return (-a if (sa or a == 32768) else a, -b if (sb or b == 32768) else b)


def single(m):
    """the class holds one reachable value: its tie degenerates"""
    return class_ends(m)[0][0] == class_ends(m)[1][0]


def roots():
    """the boundary roots R: 0 and the first classes, the i8 ceiling, the f16 denormal | normal edge, every f16 exponent edge, the
    finite | infinity | NaN edge, the sign edge, the top of the range, and 24 more from a seed"""
    edge = [0, 1, 2, 3, 180, 181, 182, 1022, 1023, 1024, 1025, 2047, 2048, 4095, 4096, 8191, 8192, 16383, 16384,
            31742, 31743, 31744, 31745, 32766, 32767, 32768, 32769, 46338, 46339, 46340]
    rng = np.random.default_rng(SEED)
    more = []
    while len(more) < 24:
        r = int(rng.integers(4, 46338))
        if r not in edge and r not in more:
            more.append(r)
    return edge + sorted(more)


R = roots()


# ---- windows and buffers --------------------------------------------------------------------------------------------------
def canon(m, seed=0):
    """the plain sample of magnitude m: (m, 0) where an i16 holds m"""
    return (m, 0) if m <= 32767 else rep(m, "min", seed)


class Window:
    def __init__(self, name, frame, mags, moved, ok):
        """mags: 240 roots; moved: {sample index: (I, Q)} for the samples that are not canon(root); ok: the reference's verdict
        (the frame comes back)"""
        self.name, self.frame, self.ok = name, frame, bool(ok)
        self.mags = np.asarray(mags, dtype=np.int64)
        self.iq = np.zeros((S.WINDOW, 2), dtype=np.int16)
        for k, m in enumerate(self.mags):
            self.iq[k] = moved[k] if k in moved else canon(int(m), k)
        self.big = bool(self.mags.max() >= F16_LIMIT)


class Buffer:
    def __init__(self, name, n):
        self.name, self.n = name, n
        self.mag = S.background(n)
        self.iq = S.to_iq(self.mag, np.int16)
        self.plants = []   # (offset, Window)
        self.notes = {}    # what a builder wants asserted about single tiles

    def plant(self, off, w):
        assert 0 <= off and off + S.WINDOW <= self.n, (self.name, off)
        assert all(off >= o + S.WINDOW or off + S.WINDOW <= o for o, _ in self.plants), (self.name, off)
        self.mag[off:off + S.WINDOW] = w.mags
        self.iq[off:off + S.WINDOW] = w.iq
        self.plants.append((off, w))

    def expected(self):
        """the frame list the reference must return: the planted frames whose window passes, by offset"""
        good = sorted((off, w.frame) for off, w in self.plants if w.ok)
        out = np.zeros(len(good), dtype=FRAME_DTYPE)
        for k, (off, frame) in enumerate(good):
            out[k] = (off, np.frombuffer(frame, dtype=np.uint8), 0, 0xFF)
        return out

    def tile_max(self, t, halo=True):
        """largest magnitude of tile t (with the halo: of every sample the tile's workgroup loads)"""
        return int(self.mag[t * TILE:(t + 1) * TILE + (HALO if halo else 0)].max(initial=0))

    def tiles(self):
        return (max(self.n - S.WINDOW, 1) + TILE - 1) // TILE

    def planted_tiles(self):
        return sorted({off // TILE for off, _ in self.plants})


def slot_offset(tile, half, slot, res):
    """plants sit 284 apart (a multiple of 4: `res` alone is the offset's residue mod 4, the sample's position in a 16-byte load),
    from 8 in run A (offsets below 4096) and in run B; slot 12 still ends inside the tile"""
    assert 0 <= slot <= 12 and 0 <= res < 4
    return tile * TILE + half * (TILE // 2) + 8 + 284 * slot + res


def plant_tile(buf, tile, windows, first_slot=0):
    """up to three windows, each at all four residues mod 4 in run A and again in run B"""
    assert len(windows) <= 3
    for j, w in enumerate(windows):
        for half in (0, 1):
            for res in range(4):
                buf.plant(slot_offset(tile, half, first_slot + 4 * j + res, res), w)


def lay_out(name, windows):
    """buffers of at most SMALL_TILES full tiles + a ragged last one, three windows per tile"""
    bufs = []
    per = 3 * SMALL_TILES
    for k in range(0, len(windows), per):
        part = windows[k:k + per]
        nt = (len(part) + 2) // 3
        b = Buffer(f"{name}[{len(bufs)}]", nt * TILE + S.WINDOW - 57)  # the last tile is 57 offsets short
        for t in range(nt):
            plant_tile(b, t, part[3 * t:3 * t + 3])
        bufs.append(b)
    return bufs


# ---- decision windows: one decisive high, one decisive low ----------------------------------------------------------------
RELATIONS = ("tie", "tie, swapped", "one class below", "one class above")
PLACES = {"preamble": (0, 1), "DF17": (16, 22)}  # (decisive high, decisive low): sample 16 stays above sample 17 (bit 1 = 1),
#                                                   sample 22 is the low of a 0 bit and stays at or below sample 23


def relation(r, rel):
    """(class and end of the decisive high, class and end of the decisive low), or None where the window cannot exist"""
    if rel in ("tie", "tie, swapped"):
        if single(r):
            return None
        return ((r, "min"), (r, "max")) if rel == "tie" else ((r, "max"), (r, "min"))
    if r + 1 > TOP:
        return None
    return ((r, "max"), (r + 1, "min")) if rel == "one class below" else ((r + 1, "min"), (r, "max"))


def decision_windows(oracle):
    """(f16-gate windows, integer-gate windows, (root, relation) pairs skipped).  The other pulses sit one class above the two
    decisive samples and the gaps one below (as far as the range goes: the f16 cases stay below 31744, the others at or below
    46340), so a is the least high, b the greatest low and the verdict is exactly a >= b."""
    f16, integer, skipped = [], [], []
    count = 0
    for r in R:
        for rel in RELATIONS:
            pick = relation(r, rel)
            if pick is None:
                skipped.append((r, rel))
                continue
            (a, ea), (b, eb) = pick
            small = max(a, b) < F16_LIMIT
            hi = min(max(a, b) + 1, F16_LIMIT - 1 if small else TOP)
            lo = max(min(a, b) - 1, 0)
            for place, (ks, kl) in PLACES.items():
                if place == "DF17" and a <= lo:
                    continue  # (a = 0: sample 16 cannot stay above sample 17)
                frame = S.frame_bytes(oracle, count % 40)
                count += 1
                mags = S.ppm(frame, hi, lo)
                mags[ks], mags[kl] = a, b
                w = Window(f"{place}: root {r}, {rel}", frame, mags, {ks: rep(a, ea, count), kl: rep(b, eb, count)}, a >= b)
                assert w.big == (not small)
                (integer if w.big else f16).append(w)
    return f16, integer, skipped


# ---- gate-choice windows: one big sample in a tile of small ones ------------------------------------------------------------
def wave_of(p):
    """the wave that loads sample p of a tile: thread (p / 4) % 256 in sweep p / 1024; the ninth sweep (the halo) is wave 0's"""
    return ((p // 4) % 256) // 64


PLACEMENTS = (("wave 0", 1024 * 1 + 256 * 0 + 37), ("wave 1", 1024 * 3 + 256 * 1 + 38), ("wave 2", 1024 * 5 + 256 * 2 + 39),
              ("wave 3", 1024 * 6 + 256 * 3 + 40), ("sample 0", 0), ("sample 8191", 8191), ("halo 0", 8192), ("halo 238", 8192 + 238))


def _last_bit_zero(oracle, first):
    idx = first
    while S.frame_bytes(oracle, idx)[-1] & 1:
        idx += 1
    return idx


def gate_choice_cases(oracle):
    """[(name, index of the big sample in the window, tile-relative index of the big sample, Window)].

    negative low: a preamble gap of 32768 or more under pulses of 100.  The reference rejects; the f16 maximum drops a negative
        pattern, so the f16 gate would pass the window.
    NaN high (preamble), as the issue states it: one preamble pulse at rep(32000, "max"), one at 100, gaps at 200.  The
        reference rejects (100 < 200).  (The scan takes the least preamble pulse as an integer in both gates, so this one
        holds in either; the DF17 form below is the one its f16 minimum3 decides.)
    NaN high (DF17): the same among the five DF17 pulses (sample 16 at 100 over a gap of 0, so bit 1 stays 1).  The f16 minimum
        would return the NaN pattern, which is above every gap as an integer.
    last sample: the big sample is the LAST sample a tile ever needs (window at the tile's last offset, its sample 239 =
        index 8192 + 238).  No gate reads it -- a gate reads 26 samples -- so no verdict can depend on it: the window passes,
        and the slicer must read that halo sample as an integer (last bit 0: sample 238 < sample 239).
    A window cannot hold a gap at a tile's sample 0 (that window starts in the tile before: the `halo 0` placement), nor a DF17
    pulse, so `sample 0` exists for the preamble NaN alone."""
    cases = []
    bigs = (("-0", (-32768, 0), 32768), ("40000", rep(40000, "max", 1), 40000), ("corner", (-32768, -32768), TOP))
    n = 0
    for pname, p in PLACEMENTS:
        if p == 8192 + 238:
            for vname, iq, m in bigs[::2]:
                frame = S.frame_bytes(oracle, _last_bit_zero(oracle, 50 + n))
                n += 1
                mags = S.ppm(frame)
                assert mags[238] == S.LO and mags[239] == S.HI
                mags[239] = m
                cases.append((f"last sample {vname}, {pname}", 239, p, Window(f"last sample {vname}", frame, mags, {239: iq}, True)))
            continue
        for j, (vname, iq, m) in enumerate(bigs):
            k = S.PRE_LOWS[(n + j) % len(S.PRE_LOWS)]
            if p - k < 0 or p - k >= TILE:
                continue
            frame = S.frame_bytes(oracle, 50 + n)
            n += 1
            mags = S.ppm(frame)
            mags[k] = m
            cases.append((f"negative low {vname} at {k}, {pname}", k, p, Window(f"negative low {vname}", frame, mags, {k: iq}, False)))
        nan = rep(32000, "max", n)
        ks = [k for k in S.PRE_HIGHS if 0 <= p - k < TILE]
        if ks:
            k = ks[n % len(ks)]
            k100 = S.PRE_HIGHS[(S.PRE_HIGHS.index(k) + 1) % 4]
            frame = S.frame_bytes(oracle, 50 + n)
            n += 1
            mags = S.ppm(frame, 300, 200)
            mags[k], mags[k100] = 32000, 100
            cases.append((f"NaN high (preamble) at {k}, {pname}", k, p, Window("NaN high (preamble)", frame, mags, {k: nan}, False)))
        ks = [k for k in (19, 21, 23, 24) if 0 <= p - k < TILE]
        if ks:
            k = ks[n % len(ks)]
            frame = S.frame_bytes(oracle, 50 + n)
            n += 1
            mags = S.ppm(frame, 300, 200)
            mags[k], mags[16], mags[17] = 32000, 100, 0
            if k == 24:
                mags[25] = 200  # (bit 5 = 1: the NaN pattern over its gap)
            cases.append((f"NaN high (DF17) at {k}, {pname}", k, p, Window("NaN high (DF17)", frame, mags, {k: nan}, False)))
    return cases


def gate_choice_buffers(oracle):
    """two tiles per case: the tile under test, whose only big sample (halo included) is the case's, and a spare one with a plain
    frame (a control: it must come back) at offset 1000.  For the halo placements the big sample is an early sample of the
    spare tile: notes[tile] = the index it must have there."""
    cases = gate_choice_cases(oracle)
    bufs, per = [], SMALL_TILES // 2
    for c0 in range(0, len(cases), per):
        part = cases[c0:c0 + per]
        b = Buffer(f"gate choice[{len(bufs)}]", 2 * len(part) * TILE + S.WINDOW + 33)
        for j, (name, k, p, w) in enumerate(part):
            t = 2 * j
            b.plant(t * TILE + p - k, w)
            b.plant((t + 1) * TILE + 1000 + (j & 3), Window("control", S.frame_bytes(oracle, 90 + (j % 8)),
                                                           S.ppm(S.frame_bytes(oracle, 90 + (j % 8))), {}, True))
            b.notes[t] = (name, p)
            if p >= TILE:
                b.notes[t + 1] = (name + " (the next tile)", p - TILE)
        bufs.append(b)
    return bufs


# ---- slicer frames --------------------------------------------------------------------------------------------------------
SLICER_ROOTS = (1, 181, 1023, 1024, 16383, 31742, 31743, 31744, 32767, 32768, 46339)


def slicer_window(oracle, idx, m, mirror):
    """ties: every 0 bit is (rep(m, "max"), rep(m, "min")): equal roots, the larger I^2 + Q^2 first; the reference slices 0.
    Every 1 bit is rep(m + 1, "min") over rep(m, "max"): one class apart and as close as two classes get.  Preamble pulses at
    m + 1, gaps at m; the DF17 part of the gate passes on ties.
    mirror: every 0 bit is the 1 bit's pair the other way round."""
    frame = S.frame_bytes(oracle, idx)
    bits = np.unpackbits(np.frombuffer(frame, dtype=np.uint8))
    mags = S.ppm(frame, m + 1, m)
    moved = {}
    for k, bit in enumerate(bits):
        s = 16 + 2 * k
        if bit:
            mags[s], mags[s + 1] = m + 1, m
            moved[s], moved[s + 1] = rep(m + 1, "min", s), rep(m, "max", s)
        elif mirror:
            mags[s], mags[s + 1] = m, m + 1
            moved[s], moved[s + 1] = rep(m, "max", s), rep(m + 1, "min", s)
        else:
            mags[s], mags[s + 1] = m, m
            moved[s], moved[s + 1] = rep(m, "max", s), rep(m, "min", s)
    return Window(f"slicer {'steps' if mirror else 'ties'} at {m}", frame, mags, moved, True)


def slicer_buffers(oracle):
    """one buffer of f16-gate frames (m + 1 below 31744), one of integer-gate frames; each frame at an odd offset in run A and at
    an even one in run B"""
    out = []
    for name, pick in (("slicer f16", lambda m: m + 1 < F16_LIMIT), ("slicer integer", lambda m: m + 1 >= F16_LIMIT)):
        ws = [slicer_window(oracle, 70 + 2 * i + mirror, m, mirror)
              for i, m in enumerate(SLICER_ROOTS) if pick(m) for mirror in (False, True)]
        nt = (len(ws) + 11) // 12
        b = Buffer(name, nt * TILE + S.WINDOW - 91)
        for j, w in enumerate(ws):
            t, slot = divmod(j, 12)
            b.plant(slot_offset(t, 0, slot, 1), w)
            b.plant(slot_offset(t, 1, slot, 2), w)
        out.append(b)
    return out


# ---- three channels, the gates mixed ----------------------------------------------------------------------------------------
def three_channels(oracle):
    """three buffers of one length: f16-gate windows only, integer-gate windows only, and the two alternating tile by tile (the
    integer tiles' plants keep clear of the 256 samples the f16 tile before them loads as its halo, and end inside their own
    tile).  Three full tiles and a ragged fourth each, with a decision window at the last offset the reference looks at."""
    f16, integer, _ = decision_windows(oracle)
    n = 3 * TILE + S.WINDOW + 300
    spread = lambda ws, k, at: [ws[(at + j * (len(ws) // k)) % len(ws)] for j in range(k)]
    bufs = []
    for c, kinds in enumerate(("fff", "iii", "fif")):
        b = Buffer(f"channel {c}", n)
        for t, kind in enumerate(kinds):
            ws = spread(f16, 9, 5 * c)[3 * t:3 * t + 3] if kind == "f" else spread(integer, 9, 7 * c)[3 * t:3 * t + 3]
            plant_tile(b, t, ws, first_slot=0 if kind == "f" else 1)
        last = (f16 if c == 0 else integer)
        b.plant(n - S.WINDOW - 1, [w for w in last if w.ok][11 * (c + 1)])
        b.notes = {t: kind for t, kind in enumerate(kinds + ("f" if c == 0 else "i"))}
        bufs.append(b)
    return bufs


_BUILT = {}


def built(oracle):
    """every buffer of this module, built once: {"f16": [...], "integer": [...], "gate choice": [...], "slicer": [...],
    "channels": [...], "skipped": [...]}; the arrays are read-only"""
    if not _BUILT:
        f16, integer, skipped = decision_windows(oracle)
        _BUILT.update({"f16": lay_out("f16 gate", f16), "integer": lay_out("integer gate", integer),
                       "gate choice": gate_choice_buffers(oracle), "slicer": slicer_buffers(oracle),
                       "channels": three_channels(oracle), "skipped": skipped,
                       "pairs": len(R) * len(RELATIONS)})
        for key in ("f16", "integer", "gate choice", "slicer", "channels"):
            for b in _BUILT[key]:
                b.iq.setflags(write=False)
                b.mag.setflags(write=False)
    return _BUILT
