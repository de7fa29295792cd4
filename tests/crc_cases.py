"""Every CRC syndrome class, planted so that each path that decides it sees all of them (tests/test_crc_cases.py on the CPU,
tests/test_gpu_crc_paths.py and tests/ab_cases.py on the device).

A gate survivor becomes a frame by one verdict on s = CRC24(data) ^ crc_field: clean (s == 0), repaired (s is the syndrome
of one of the 88 data bits) or dropped (crc.rs:49-65).  The device has two implementations of that verdict (finish_record:
byte table + binary search over the sorted syndromes; count_candidate: XOR of the per-bit table, used where a tile lost its
slots and is only counted), and which lanes run them depends on the tile's survivor count.  So the cases here are frame
CLASSES, each with the verdict it must get, and LAYOUTS that put every class into tiles of one survivor-count band.

The model (SYN, syndrome, verdict, model_list) is built from the generator polynomial alone; nothing is taken from the
library.  Buffers are magnitudes as in tests/survivor_cases.py (I = magnitude, Q = 0: both sample types see the same values).

Classes, all derived from clean frames F = survivor_cases.frame_bytes(oracle, i):
  clean      F itself: status 0.
  flip j     data bit j of F flipped, j = 0..87.  j = 5..87 come back (status 1, fixed_bit j, bytes F).  j = 0..4 break the
             DF17 pattern, never pass the gate and must not appear (`absent`).
  tie p      both samples of DF17 pair p (0 or 4) at 60: the gate passes on >=, the strict slicer reads the tie as 0, and the
             frame comes back (1, p, F).  That is the only way to a fixed_bit below 5, and bits 1..3 cannot be reached at
             all: they are 0 in DF17, and a sliced 1 there fails the gate.
  crc j      CRC-field bit j = 88..111 flipped: s = 1 << (111 - j), never a data syndrome, dropped.
  near s     CRC field XORed with s, for s in {1, 0xFFFFFF} and t - 1, t + 1 of every data syndrome t (178 values, none of
             them a data syndrome): the edges of the binary search (1 lies below every entry, 0xFFFFFF above every entry,
             where the search lands on the table's padding).  Dropped.
  alias i>k  data bit i flipped and the CRC field XORed with SYN[i] ^ SYN[k]: the syndrome is SYN[k], the reference
             "repairs" bit k and returns a WRONG frame with status 1, fixed_bit k.  So must the device.
  stub       survivor_cases.stub(): a survivor that takes a slot and is no frame."""
from collections import namedtuple

import numpy as np

from tests import survivor_cases as S

GEN = 0x1FFF409
TIE = 60
N_BASE = 8  # clean base frames the classes are derived from, in turn


def _polymod(v):
    """v (a polynomial over GF(2), bit k = x^k) mod the generator"""
    while v.bit_length() > 24:
        v ^= GEN << (v.bit_length() - 25)
    return v


SYN = [_polymod(1 << (111 - j)) for j in range(112)]  # syndrome of frame bit j (MSB first): x^(111-j) mod GEN
DATA_SYN = SYN[:88]
BIT_OF = {s: j for j, s in enumerate(DATA_SYN)}
SORTED_SYN = sorted(DATA_SYN)
NEIGHBOURS = sorted({1, 0xFFFFFF} | {t + d for t in DATA_SYN for d in (-1, 1)})
# the least every layout carries: below and above all entries, and around the first, the last and the two middle entries
EDGE_NEIGHBOURS = sorted({1, 0xFFFFFF} | {SORTED_SYN[i] + d for i in (0, 43, 44, 87) for d in (-1, 1)})
ALIASES = ((10, 70), (87, 5), (40, 41), (6, 86))


def syndrome(frame14):
    """CRC24(data) ^ crc_field = the 112-bit frame as a polynomial, mod the generator"""
    return _polymod(int.from_bytes(bytes(frame14), "big"))


def flip(frame14, j):
    b = bytearray(frame14)
    b[j >> 3] ^= 0x80 >> (j & 7)
    return bytes(b)


def xor_crc(frame14, s):
    b = bytes(frame14)
    return b[:11] + (int.from_bytes(b[11:], "big") ^ s).to_bytes(3, "big")


def verdict(frame14):
    """(status, fixed_bit, bytes) of a sliced frame, or None where it is dropped (crc.rs:49-65)"""
    s = syndrome(frame14)
    if s == 0:
        return 0, 0xFF, bytes(frame14)
    if s in BIT_OF:
        return 1, BIT_OF[s], flip(frame14, BIT_OF[s])
    return None


def model_list(mag):
    """[(offset, status, fixed_bit, bytes)] of a whole magnitude buffer: the reference gate, the strict slicer (a pair is a 1
    only where its first sample is larger), the verdict"""
    mag = np.asarray(mag, dtype=np.int64)
    rows = []
    for off in np.nonzero(S.gate(mag))[0]:
        w = mag[off + 16:off + S.WINDOW]
        v = verdict(np.packbits(w[0::2] > w[1::2]).tobytes())
        if v is not None:
            rows.append((int(off),) + v)
    return rows


# kind: clean | repaired | dropped (a survivor that is no frame) | absent (no survivor at all)
Item = namedtuple("Item", "cls kind mags expect")  # expect = (status, fixed_bit, bytes), or None: nothing comes out
Plant = namedtuple("Plant", "off item")
Layout = namedtuple("Layout", "path tile n_samples plants band")


def _clean(f):
    return Item("clean", "clean", S.ppm(f), (0, 0xFF, f))


def _data_flip(f, j):
    if j < 5:
        return Item("flip %d" % j, "absent", S.ppm(flip(f, j)), None)
    return Item("flip %d" % j, "repaired", S.ppm(flip(f, j)), (1, j, f))


def _tie(f, pair):
    m = S.ppm(f)
    m[16 + 2 * pair] = m[17 + 2 * pair] = TIE
    return Item("tie %d" % pair, "repaired", m, (1, pair, f))


def _crc_flip(f, j):
    return Item("crc %d" % j, "dropped", S.ppm(flip(f, j)), None)


def _near(f, s):
    return Item("near %06X" % s, "dropped", S.ppm(xor_crc(f, s)), None)


def _alias(f, i, k):
    r = xor_crc(flip(f, i), SYN[i] ^ SYN[k])
    return Item("alias %d>%d" % (i, k), "repaired", S.ppm(r), (1, k, flip(r, k)))


STUB = Item("stub", "dropped", S.stub(), None)


def work_items(oracle, path):
    """every class but clean and stub, repaired and dropped ones evenly interleaved, each on one of N_BASE base frames"""
    base = [S.frame_bytes(oracle, i) for i in range(N_BASE)]
    makers = [lambda f, j=j: _data_flip(f, j) for j in range(5, 88)]
    makers += [lambda f, p=p: _tie(f, p) for p in (0, 4)]
    makers += [lambda f, i=i, k=k: _alias(f, i, k) for i, k in ALIASES]
    others = [lambda f, j=j: _crc_flip(f, j) for j in range(88, 112)]
    others += [lambda f, s=s: _near(f, s) for s in (NEIGHBOURS if path == "sparse" else EDGE_NEIGHBOURS)]
    for j in range(5):  # (spread out: no tile's dropped frames are these alone)
        others.insert(3 + 7 * j, lambda f, j=j: _data_flip(f, j))
    keyed = [(i / len(makers), 0, m) for i, m in enumerate(makers)] + [(i / len(others), 1, m) for i, m in enumerate(others)]
    keyed.sort(key=lambda t: t[:2])
    return [m(base[i % N_BASE]) for i, (_, _, m) in enumerate(keyed)]


# path: (band of survivors per tile, work frames per tile, planted survivors per tile)
SPECS = {
    "sparse": ((1, 16), 12, 0),   # frames only (three short of the band's end: a flipped frame's image can pass the gate a
                                  # second time); a clean one in every tile, one stub in the last
    "quota": ((17, 32), 22, 24),
    "pool": ((33, 64), 22, 48),
    "dense": ((65, 128), 15, 96),  # its first tile has 136: band (129, ...)
}
PATHS = tuple(SPECS)
DENSE_FIRST = 136


def _tile_plants(tile0, items, n_stubs):
    """frames 250 apart from offset 5 of the tile, the stubs 32 apart, spread evenly behind the frames (so that the valid frames
    of a dense tile lie in every chunk of its ordered list)"""
    plants, pos = [], tile0 + 5
    for i, it in enumerate(items):
        plants.append(Plant(pos, it))
        pos += 250
        for _ in range((i + 1) * n_stubs // len(items) - i * n_stubs // len(items)):
            plants.append(Plant(pos, STUB))
            pos += 32
    return plants, pos


def cases(oracle, tile, path):
    """the Layout of one path at one tile length: whole tiles only, n_samples = tiles * tile + 240; band[t] = (lo, hi) of tile t"""
    (lo, hi), per_tile, target = SPECS[path]
    work = work_items(oracle, path)
    plants, band = [], []
    for t, first in enumerate(range(0, len(work), per_tile)):
        items = [_clean(S.frame_bytes(oracle, N_BASE + t))] + work[first:first + per_tile]
        survivors = sum(it.kind != "absent" for it in items)
        want = DENSE_FIRST if (path == "dense" and t == 0) else target
        n_stubs = max(want - survivors, 0)
        if path == "sparse" and first + per_tile >= len(work):
            n_stubs = 1
        p, end = _tile_plants(t * tile, items, n_stubs)
        assert end <= (t + 1) * tile, (path, tile, t, end)  # every plant starts inside its own tile
        plants += p
        band.append((129, tile) if (path == "dense" and t == 0) else (lo, hi))
    return Layout(path, tile, len(band) * tile + S.WINDOW, plants, band)


def layout(oracle, tile, path):
    """(n_samples, plants) as survivor_cases.build takes them"""
    c = cases(oracle, tile, path)
    return c.n_samples, [(p.off, p.item.mags) for p in c.plants]


def magnitudes(c, n=None):
    """the buffer of a Layout (n: padded with background to that length)"""
    return S.build(c.n_samples if n is None else n, [(p.off, p.item.mags) for p in c.plants])


def check_figures(c, want):
    """what the issue measured for every class, re-asserted on the oracle's list `want` for the frames this layout uses:
    every plant comes back with exactly its class's (status, fixed_bit, bytes), or not at all"""
    at = {}
    for r in want:
        at.setdefault(int(r["offset"]), []).append((int(r["status"]), int(r["fixed_bit"]), r["bytes"].tobytes()))
    for p in c.plants:
        got = at.get(p.off, [])
        assert got == ([p.item.expect] if p.item.expect else []), (c.path, p.off, p.item.cls, got)


def check_bands(c, mag):
    counts = S.survivors_per_tile(mag, c.tile)[:len(c.band)]
    assert len(counts) == len(c.band)
    for t, (k, (lo, hi)) in enumerate(zip(counts, c.band)):
        assert lo <= k <= hi, (c.path, c.tile, t, k, (lo, hi))
    return counts


def check_mix(c):
    """no tile of the quota, pool and dense layouts is all one class: repaired, dropped and clean frames side by side"""
    if c.path == "sparse":
        return
    for t in range(len(c.band)):
        kinds = {p.item.kind for p in c.plants if p.off // c.tile == t and p.item is not STUB}
        assert {"clean", "repaired", "dropped"} <= kinds, (c.path, t, kinds)


def check_coverage(c):
    """what every layout carries"""
    names = {p.item.cls for p in c.plants}
    need = {"clean", "stub", "tie 0", "tie 4"} | {"flip %d" % j for j in range(88)} | {"crc %d" % j for j in range(88, 112)}
    need |= {"alias %d>%d" % a for a in ALIASES}
    need |= {"near %06X" % s for s in (NEIGHBOURS if c.path == "sparse" else EDGE_NEIGHBOURS)}
    assert need <= names, (c.path, sorted(need - names))


def valid_per_tile(want, tile, n_tiles):
    """the oracle's valid frames per tile"""
    return np.bincount((want["offset"] // tile).astype(np.int64), minlength=n_tiles)[:n_tiles]
