"""Hand-built PPM buffers with a known number of gate survivors per tile (tests/test_gpu_survivor_list.py).

Everything is built as MAGNITUDES (I = magnitude, Q = 0, so both sample types see exactly these values) over a background
that alternates 0 / 10 and passes the gate nowhere.  A planted FRAME is a whole valid DF17 frame (preamble, 112 PPM bit
pairs, CRC from the oracle): a survivor that also comes back in the output.  A planted STUB is the gate's 26 samples only
(preamble + the five DF17 bit pairs): a survivor that takes a slot and is dropped by the CRC.  gate() is the reference gate
(demod.rs:17-57) over a whole magnitude array, so a test can assert the survivor count of every tile before it looks at
what the device made of it."""
import numpy as np

WINDOW = 240
HI, LO, BG = 100, 0, 10
PRE_HIGHS = (0, 2, 7, 9)
PRE_LOWS = (1, 3, 4, 5, 6, 8, 10, 11, 12, 13, 14, 15)
DF_HIGHS = (16, 19, 21, 23, 24)  # DF17 = 1 0 0 0 1, pair k at samples 16 + 2k, 17 + 2k
DF_LOWS = (17, 18, 20, 22, 25)


_CLEAN = []  # seeds of frames_bytes whose PPM image holds no second window that passes the gate


def _frame_of_seed(oracle, seed):
    rng = np.random.default_rng(1000 + seed)
    data = bytes([0x8D]) + bytes(rng.integers(0, 256, size=10, dtype=np.uint8))
    crc = oracle.get_adsb_crc(data)
    return data + bytes([(crc >> 16) & 0xFF, (crc >> 8) & 0xFF, crc & 0xFF])


def frame_bytes(oracle, idx):
    """the idx-th valid 14-byte DF17 frame (0x8D, ten seeded bytes, CRC-24) that is exactly ONE gate survivor when planted
    into the background, at an even or an odd offset: pulse patterns inside a frame can pass the gate a second time, and the
    cases here need exact counts"""
    seed = _CLEAN[-1] + 1 if _CLEAN else 0
    while len(_CLEAN) <= idx:
        f = ppm(_frame_of_seed(oracle, seed))
        if all(gate(build(800, [(off, f)])).sum() == 1 for off in (300, 301)):
            _CLEAN.append(seed)
        seed += 1
    return _frame_of_seed(oracle, _CLEAN[idx])


def ppm(frame, hi=HI, lo=LO):
    """the 240 magnitudes of one frame: bit 1 = (hi, lo), bit 0 = (lo, hi), MSB first"""
    m = np.full(WINDOW, lo, dtype=np.int64)
    m[list(PRE_HIGHS)] = hi
    bits = np.unpackbits(np.frombuffer(frame, dtype=np.uint8))
    m[16::2] = np.where(bits == 1, hi, lo)
    m[17::2] = np.where(bits == 1, lo, hi)
    return m


def stub(hi=HI, lo=LO):
    """the gate's own 26 samples: preamble and the five DF17 pairs"""
    return ppm(bytes([0x88]) + bytes(13), hi, lo)[:26]


def background(n):
    m = np.zeros(n, dtype=np.int64)
    m[1::2] = BG
    return m


def build(n, plants):
    """magnitudes of a buffer of n samples; plants = [(offset, array of magnitudes)] (clipped at the buffer's end)"""
    m = background(n)
    for off, v in plants:
        v = np.asarray(v)[:max(0, n - off)]
        m[off:off + len(v)] = v
    return m


def to_iq(mag, dtype):
    iq = np.zeros((len(mag), 2), dtype=dtype)
    iq[:, 0] = mag
    return iq


def gate(mag):
    """bool per offset 0 .. len - 241: the reference gate (ties pass: >=)"""
    mag = np.asarray(mag, dtype=np.int64)
    n = len(mag) - WINDOW
    if n <= 0:
        return np.zeros(0, dtype=bool)
    at = lambda k: mag[k:k + n]
    ph = np.minimum.reduce([at(k) for k in PRE_HIGHS])
    pl = np.maximum.reduce([at(k) for k in PRE_LOWS])
    dh = np.minimum.reduce([at(k) for k in DF_HIGHS])
    dl = np.maximum.reduce([at(k) for k in DF_LOWS])
    return (ph >= pl) & (dh >= dl)


def survivors_per_tile(mag, tile):
    g = gate(mag)
    return [int(g[t:t + tile].sum()) for t in range(0, max(len(g), 1), tile)]


def tile_with(oracle, tile0, k, first):
    """plants for exactly k survivors in the tile that starts at tile0 (a multiple of the tile length): up to 16 whole frames
    from offset 5, 250 apart, then stubs from offset 4100, 32 apart.  Frames are drawn from frame_bytes(first), (first + 1), ...;
    one whose neighbourhood would pass the gate a second time (a window across two frames) is passed over."""
    local, idx = [], first
    for j in range(min(k, 16)):
        while True:
            cand = local + [(5 + 250 * j, ppm(frame_bytes(oracle, idx)))]
            idx += 1
            if gate(build(8192 + WINDOW, cand)).sum() == len(cand):
                local = cand
                break
    local += [(4100 + 32 * j, stub()) for j in range(k - len(local))]
    assert gate(build(8192 + WINDOW, local)).sum() == k
    return [(tile0 + off, v) for off, v in local]


# The DF17 part of the gate, plain cases and ties: one clean frame with a few of its DF17 samples moved (sample index -> magnitude).  None of them changes
# a sliced bit (a pair's order stays, a tie slices as 0 where the frame has a 0), so a window the gate rejects would come
# back as a valid frame if the device let it through.  True = the gate passes (min of five highs >= max of five lows).
DF17_VARIANTS = (
    ("plain", {}, True),
    ("pairs 1-3 pass, low of pair 4 above a high of pair 1", {16: 50, 22: 60}, False),
    ("pairs 1-3 pass, low of pair 5 above a high of pair 1", {16: 50, 25: 60}, False),
    ("pairs 1-3 pass, high of pair 4 below a low of pair 2", {23: 50, 18: 60}, False),
    ("pairs 1-3 pass, high of pair 5 below a low of pair 3", {24: 50, 20: 60}, False),
    ("pairs 4-5 pass, low of pair 2 above a high of pair 1", {16: 50, 18: 60}, False),
    ("pairs 4-5 pass, low of pair 3 above a high of pair 2", {19: 50, 20: 60}, False),
    ("tie inside pairs 1-3", {16: 60, 18: 60}, True),
    ("tie inside one pair", {19: 60, 18: 60}, True),
    ("tie between a high of pair 1 and a low of pair 4", {16: 60, 22: 60}, True),
    ("tie between a high of pair 4 and a low of pair 2", {23: 60, 18: 60}, True),
    ("tie between a high of pair 5 and a low of pair 5's neighbour", {24: 60, 22: 60}, True),
    ("all tied but the two lows a sliced 1 needs lower", {16: 60, 17: 59, 18: 60, 19: 60, 20: 60, 21: 60, 22: 60, 23: 60, 24: 60,
                                                          25: 59}, True),
    ("all ten tied (bits 1 and 5 then slice as 0: two flips, no valid frame, but a survivor)",
     {16: 60, 17: 60, 18: 60, 19: 60, 20: 60, 21: 60, 22: 60, 23: 60, 24: 60, 25: 60}, True),
)


def df17_plants(oracle, tile, first=40):
    """every variant once in the first half of a tile (run A of a lane) and once in the second (run B), 280 apart, at odd and
    even offsets; returns (plants, number that pass)"""
    plants, n_pass = [], 0
    for half in (0, 1):
        for i, (_, moves, ok) in enumerate(DF17_VARIANTS):
            m = ppm(frame_bytes(oracle, first + i))
            for k, v in moves.items():
                m[k] = v
            plants.append((half * (tile // 2) + 7 + 281 * i, m))
            n_pass += ok
    return plants, n_pass
