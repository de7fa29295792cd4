"""Hostile Mode-S traffic for the tracker tests, and a census of what it reaches.

tests/traffic.py makes well-behaved traffic (consistent even / odd pairs at moderate latitudes, type codes 4, 11 and 19,
times drawn as floats).  This generator is built from NAMED CASES, each on ICAO addresses of its own so that a failure
names its case, and it returns integer SAMPLE positions, so a test forms every time exactly as the library does:
float(sample_base + offset) * seconds_per_sample.

  cpr_*   even / odd pairs chosen for a branch of cpr.rs: uniform 17-bit fields; pairs the decode refuses (the zone
          counts of the two latitudes differ); latitude exactly 0, +87 and -87; the `> 270` fold; one-zone and two-zone
          latitudes; longitudes that need the +-180 loops; pairs where the `latitude - 1.0` quirk changes the zone
          count.  Every pair in both orders (even first on one ICAO, odd first on the next).
  win_*   partners exactly round(10 / sps) samples apart, one sample less and one more, at stream positions near 0,
          across 2^40 and above 2^53 (where the u64 -> f64 conversion rounds); a partner outside the window with
          identification, velocity, unknown and same-format position frames of the same aircraft inside it, and the
          same with the partner just inside.
  mix     every type code 0-31, TC 19 of every subtype, all 64 six-bit callsign characters, altitude codes with the Q
          bit set and clear including 0 and 0xFFF, and first bytes other than 0x8D (host lists only: the demodulator
          passes nothing but DF 17).  Every CRC is correct, so the DF 17 part can also be modulated.
  seg_*   segment shapes of the sort by ICAO: ICAO 000000, FFFFFF, 7FFFFF / 800000, a run of adjacent ICAOs, many
          aircraft heard exactly once, segments of 255, 256 and 257 frames, one segment that is a large share of the
          list, and a Zipf-like spread for the rest; the frames carry uniformly random ME bytes.

census() replays a traffic through the ORACLE alone and counts per case what was reached; check_census() holds the
floors that keep a test from passing without having tested its case.  One condition protects the device: no aircraft
has more than 256 frames inside any 10 s window (the pairs step walks back frame by frame to its partner or to the
window's edge); the generator asserts it.
"""
import math

import numpy as np

from tests.traffic import ident_frame, position_frame
from tests.velocity_traffic import random_velocity_frame

SAMPLE_PERIODS = (0.5e-6, 1.0 / 2.4e6, 1e-3, 2.0 ** -20)
REGIONS = ("near_0", "across_2^40", "above_2^53")
WINDOW_S = 10.0
MAX_IN_WINDOW = 256
OTHER_FIRST_BYTES = (0x8F, 0x88, 0x8A, 0x5D, 0xA0, 0x00, 0xFF, 0x02, 0x28)   # 0x88-0x8F are DF 17 with another CA
CPR_CASES = ("cpr_uniform", "cpr_refused", "cpr_lat0", "cpr_lat87p", "cpr_lat87n", "cpr_fold", "cpr_one_zone",
             "cpr_two_zone", "cpr_lon_wrap", "cpr_quirk")
WIN_CASES = ("win_exact", "win_inside", "win_outside", "win_outside_fill", "win_inside_fill")
SEG_CASES = ("seg_special", "seg_adjacent", "seg_single", "seg_255_256_257", "seg_big", "seg_zipf")
CASES = CPR_CASES + WIN_CASES + ("mix",) + SEG_CASES
# what a cpr_* case is there to reach (a key of classify()); cpr_uniform is counted by its evaluations
CPR_TARGET = {"cpr_refused": "refused", "cpr_lat0": "lat0", "cpr_lat87p": "lat87p", "cpr_lat87n": "lat87n",
              "cpr_fold": "fold", "cpr_one_zone": "one_zone", "cpr_two_zone": "two_zone", "cpr_lon_wrap": "lon_wrap",
              "cpr_quirk": "quirk"}
EXACT_LATITUDE_CASES = ("cpr_lat0", "cpr_lat87p", "cpr_lat87n")

_POLY = 0xFFF409
_CRC_TABLE = np.zeros(256, dtype=np.uint32)
for _b in range(256):
    _c = _b << 16
    for _ in range(8):
        _c = ((_c << 1) ^ _POLY if _c & 0x800000 else _c << 1) & 0xFFFFFF
    _CRC_TABLE[_b] = _c


def crc24(data):
    """The Mode-S CRC of the first 11 bytes of every row of a (n, >= 11) uint8 array (crc.rs:10-40, table-driven);
    hostile_traffic() checks it against oracle.get_adsb_crc."""
    crc = np.zeros(len(data), dtype=np.uint32)
    for k in range(11):
        crc = ((crc << np.uint32(8)) & np.uint32(0xFFFFFF)) ^ _CRC_TABLE[((crc >> np.uint32(16)) ^ data[:, k]) & 0xFF]
    return crc


def seal(frames):
    """Writes the correct CRC into bytes 11-13 of every row of a (n, 14) uint8 array, in place."""
    crc = crc24(frames)
    frames[:, 11], frames[:, 12], frames[:, 13] = (crc >> 16) & 0xFF, (crc >> 8) & 0xFF, crc & 0xFF
    return frames


def with_first_byte(frame, first):
    """The same frame under another first byte (downlink format / capability), with its CRC made right again."""
    a = np.frombuffer(bytes([first]) + bytes(frame)[1:], dtype=np.uint8).reshape(1, 14).copy()
    return bytes(seal(a)[0])


def classify(oracle, even_lat, even_lon, odd_lat, odd_lon, first_is_odd):
    """What ONE evaluation of cpr.rs:135-147 reaches, from the oracle's own pieces (calculate_latitude,
    calc_num_zones): a dict of booleans.  A refused pair reaches nothing but `refused` and `fold`."""
    lat, e_lat, o_lat = oracle.calculate_latitude(even_lat, odd_lat, first_is_odd)
    raw = e_lat if first_is_odd else o_lat
    out = dict.fromkeys(("refused", "fold", "lat0", "lat87p", "lat87n", "one_zone", "two_zone", "quirk", "lon_wrap"),
                        False)
    out["fold"] = raw > 270.0
    if oracle.calc_num_zones(e_lat) != oracle.calc_num_zones(o_lat):
        out["refused"] = True
        return out
    nl = oracle.calc_num_zones(lat)
    nz = nl if first_is_odd else max(oracle.calc_num_zones(lat - 1.0), 1)        # sic: latitude - 1.0 (cpr.rs:100)
    out["lat0"], out["lat87p"], out["lat87n"] = lat == 0.0, lat == 87.0, lat == -87.0
    out["one_zone"], out["two_zone"] = nl == 1, nl == 2
    out["quirk"] = (not first_is_odd) and nz != nl
    ce, co = even_lon / 131072.0, odd_lon / 131072.0
    m = math.floor(ce * float(nl - 1) - co * float(nl) + 0.5)
    lon = (360.0 / nz) * (math.fmod(m, float(nz)) + (ce if first_is_odd else co))
    out["lon_wrap"] = lon < -180.0 or lon > 180.0
    return out


def too_old(x_i, x_j, sps):
    """aircraft.rs:68-70 on the header's times: each time is ONE rounded product of the sample position."""
    return abs(float(x_i) * sps - float(x_j) * sps) > WINDOW_S


class Traffic:
    """samples (uint64, ascending) and frames ((n, 14) uint8) of one list; case[k] indexes CASES; cpr_pairs and
    window_pairs hold list indices: (case, first, second) and dicts with case / region / delta / first / second /
    inside (indices of the fill frames between the two)."""

    def __init__(self, sps, samples, frames, case, cpr_pairs, window_pairs):
        self.sps, self.samples, self.frames, self.case = sps, samples, frames, case
        self.cpr_pairs, self.window_pairs = cpr_pairs, window_pairs
        self.icao = (frames[:, 1].astype(np.uint32) << 16) | (frames[:, 2].astype(np.uint32) << 8) | frames[:, 3]

    def __len__(self):
        return len(self.samples)

    def __iter__(self):
        """(sample, frame_bytes), ascending in sample"""
        return ((int(s), bytes(f)) for s, f in zip(self.samples, self.frames))

    def times(self, base=0):
        """float(base + sample) * sps of every frame, as the library forms them"""
        return (self.samples + np.uint64(base)).astype(np.float64) * self.sps

    def frame_array(self, dtype, lo=0, hi=None, base=0):
        """frames [lo, hi) as a FRAME_DTYPE array with offset = sample - base"""
        hi = len(self) if hi is None else hi
        out = np.zeros(hi - lo, dtype=dtype)
        out["offset"] = self.samples[lo:hi] - np.uint64(base)
        out["bytes"] = self.frames[lo:hi]
        out["fixed_bit"] = 0xFF
        return out

    def select(self, mask):
        """The sub-list mask picks (a boolean array), pair indices dropped."""
        return Traffic(self.sps, self.samples[mask], self.frames[mask], self.case[mask], [], [])


class _Builder:
    def __init__(self, oracle, rng, sps):
        self.oracle, self.rng, self.sps = oracle, rng, sps
        self.samples, self.frames, self.case = [], [], []       # python ints / bytes / case index, in creation order
        self.bulk = []                                          # (samples u64, frames (n, 14), case index)
        self.cpr_pairs, self.window_pairs = [], []
        self.next_icao = {c: 0x100000 + 0x40000 * k for k, c in enumerate(CASES)}

    def icao(self, case):
        self.next_icao[case] += 1
        return self.next_icao[case] - 1

    def add(self, case, sample, frame):
        assert len(frame) == 14 and sample >= 0
        self.samples.append(int(sample))
        self.frames.append(bytes(frame))
        self.case.append(CASES.index(case))
        return len(self.samples) - 1

    def at(self, seconds):
        return int(round(seconds / self.sps))


def decodes_both_orders(oracle, f):
    return all(oracle.geographic_position(*f, first_is_odd) is not None for first_is_odd in (False, True))


def draw_fields(rng):
    return tuple(int(x) for x in rng.integers(0, 1 << 17, size=4))          # even lat, even lon, odd lat, odd lon


def _cpr_cases(b, span_s, n_pairs, n_exact):
    """Each chosen field set on two ICAOs: even first, and odd first."""
    oracle, rng = b.oracle, b.rng
    for case in CPR_CASES:
        chosen = []
        if case == "cpr_uniform":
            chosen = [draw_fields(rng) for _ in range(n_pairs)]
        elif case == "cpr_lat0":                               # latitude index 0 and both fractions 0: exactly 0.0
            chosen = [(0, 0, 0, 0)] * min(4, n_exact) + [(0, int(rng.integers(0, 1 << 17)), 0, int(rng.integers(0, 1 << 17)))
                                                         for _ in range(n_exact - 4)]
        elif case in ("cpr_lat87p", "cpr_lat87n"):             # the newer message even: 6 x (14 + 1/2), 6 x (-15 + 1/2)
            o_lat = 32769 if case == "cpr_lat87p" else 98304
            chosen = [(65536, int(rng.integers(0, 1 << 17)), o_lat, int(rng.integers(0, 1 << 17)))
                      for _ in range(n_exact)]
        else:
            want = CPR_TARGET[case]
            for _ in range(400_000):
                f = draw_fields(rng)
                # the quirk needs the newer message odd; the others are taken as the even-first order finds them
                if classify(oracle, *f, first_is_odd=False)[want]:
                    chosen.append(f)
                    if len(chosen) == n_pairs:
                        break
            assert len(chosen) == n_pairs, case
        for f in chosen:
            for odd_first in (False, True):
                icao = b.icao(case)
                t0 = rng.uniform(0.0, span_s - 6.0)
                x0 = b.at(t0)
                x1 = max(b.at(t0 + rng.uniform(0.001, 5.0)), x0 + 1)
                alt = int(rng.integers(0, 1 << 12))
                even = position_frame(oracle, icao, False, f[0], f[1], alt_code=alt, tc=int(rng.integers(9, 19)))
                odd = position_frame(oracle, icao, True, f[2], f[3], alt_code=alt, tc=int(rng.integers(9, 19)))
                first, second = (odd, even) if odd_first else (even, odd)
                b.cpr_pairs.append((case, b.add(case, x0, first), b.add(case, x1, second)))
    for o_lat, lat in ((32769, 87.0), (98304, -87.0)):         # exact only with the EVEN message newer; both decode
        assert oracle.calculate_latitude(65536, o_lat, True)[0] == lat
        assert oracle.geographic_position(65536, 0, o_lat, 0, True) is not None


def _window_cases(b, n_each):
    """Per region and case n_each aircraft; partners D + delta samples apart, D = round(10 / sps)."""
    oracle, rng, sps = b.oracle, b.rng, b.sps
    D = int(round(WINDOW_S / sps))
    bases = {"near_0": 0, "across_2^40": (1 << 40) - D // 2, "above_2^53": (1 << 53) + (1 << 20) + 1}
    delta_of = {"win_exact": 0, "win_inside": -1, "win_outside": 1, "win_outside_fill": 1, "win_inside_fill": 0}
    for region in REGIONS:
        slot = 0
        for case in WIN_CASES:
            for k in range(n_each):
                f = draw_fields(rng)
                while not decodes_both_orders(oracle, f):
                    f = draw_fields(rng)
                icao = b.icao(case)
                odd_first = bool(k & 1)
                x0 = bases[region] + 7 * slot                  # 7: odd and even positions (above 2^53 the odd ones round)
                slot += 1
                x1 = x0 + D + delta_of[case]
                even = position_frame(oracle, icao, False, f[0], f[1], alt_code=int(rng.integers(0, 1 << 12)))
                odd = position_frame(oracle, icao, True, f[2], f[3], alt_code=int(rng.integers(0, 1 << 12)))
                first, second = (odd, even) if odd_first else (even, odd)
                rec = {"case": case, "region": region, "delta": delta_of[case], "first": b.add(case, x0, first),
                       "inside": []}
                if case.endswith("_fill"):                     # what the walk has to pass on its way to the partner
                    g = draw_fields(rng)
                    same = position_frame(oracle, icao, not odd_first, g[0] if odd_first else g[2],
                                          g[1] if odd_first else g[3])       # the NEW message's format
                    unknown = bytes(seal(np.frombuffer(bytes([0x8D]) + icao.to_bytes(3, "big") + bytes([29 << 3]) +
                                                       bytes(rng.integers(0, 256, size=9, dtype=np.uint8)),
                                                       dtype=np.uint8).reshape(1, 14).copy())[0])
                    fill = [ident_frame(oracle, icao, list(rng.integers(0, 64, size=8))),
                            random_velocity_frame(oracle, rng, icao), unknown, same]
                    for q, fr in enumerate(fill):
                        rec["inside"].append(b.add(case, x0 + (q + 1) * (D // 5), fr))
                rec["second"] = b.add(case, x1, second)
                b.window_pairs.append(rec)


def _mix_case(b, span_s, n_per_tc):
    oracle, rng = b.oracle, b.rng
    icaos = [b.icao("mix") for _ in range(8)]
    frames = []
    for tc in range(32):                                       # every type code, random ME bits behind it
        for _ in range(n_per_tc):
            me = bytearray(rng.integers(0, 256, size=7, dtype=np.uint8))
            me[0] = (tc << 3) | (me[0] & 7)
            frames.append(bytes([0x8D]) + int(rng.choice(icaos)).to_bytes(3, "big") + bytes(me) + bytes(3))
    frames = [bytes(f) for f in seal(np.frombuffer(b"".join(frames), dtype=np.uint8).reshape(-1, 14).copy())]
    subtypes = set()
    for _ in range(20 * n_per_tc):                             # TC 19, every subtype 0-7 and every kind of raw field
        frames.append(random_velocity_frame(oracle, rng, int(rng.choice(icaos))))
        subtypes.add(frames[-1][4] & 7)
    assert n_per_tc < 8 or subtypes == set(range(8))
    for rep in range(min(4, n_per_tc)):                        # all 64 six-bit characters (msgs.rs:150-177)
        for tc in (1, 2, 3, 4):
            for k in range(8):
                chars = [(8 * k + j + rep) & 63 for j in range(8)]
                fr = ident_frame(oracle, int(rng.choice(icaos)), chars)
                frames.append(with_first_byte(fr[:4] + bytes([(tc << 3) | (fr[4] & 7)]) + fr[5:], 0x8D))
    for alt in (0, 0xFFF, 0x010, 0xFEF, 0x7FF, 0x800, 0x00F, 0xFF0) + tuple(int(x) for x in rng.integers(0, 1 << 12, n_per_tc)):
        for q in (0, 1):                                       # the Q bit is bit 4 of the 12-bit code (msgs.rs:71)
            code = (alt & ~0x10) | (q << 4)
            f = draw_fields(rng)
            odd = bool(rng.integers(0, 2))
            frames.append(position_frame(oracle, int(rng.choice(icaos)), odd, f[2] if odd else f[0],
                                         f[3] if odd else f[1], alt_code=code, tc=int(rng.integers(9, 19))))
    for fr in frames:
        if rng.random() < 0.1:                                 # host lists carry whatever first byte they are given
            fr = with_first_byte(fr, int(rng.choice(OTHER_FIRST_BYTES)))
        b.add("mix", b.at(rng.uniform(0.0, span_s)), fr)


def _random_frames(rng, icao, other_first_share=0.0):
    """One frame of uniformly random ME bytes per entry of icao (uint32 array), DF 17 unless drawn otherwise."""
    n = len(icao)
    fr = np.zeros((n, 14), dtype=np.uint8)
    fr[:, 0] = 0x8D
    if other_first_share > 0:
        other = rng.random(n) < other_first_share
        fr[other, 0] = rng.choice(np.array(OTHER_FIRST_BYTES, dtype=np.uint8), size=int(other.sum()))
    fr[:, 1], fr[:, 2], fr[:, 3] = (icao >> 16) & 0xFF, (icao >> 8) & 0xFF, icao & 0xFF
    fr[:, 4:11] = rng.integers(0, 256, size=(n, 7), dtype=np.uint8)
    return seal(fr)


def _segment_cases(b, span_s, n_single, n_big, n_zipf_aircraft, n_zipf_frames, edge_lengths):
    rng, sps = b.rng, b.sps
    span = b.at(span_s)

    def evenly(n):                                             # n positions spread over the span, jittered
        step = span / n
        return (np.arange(n) * step + rng.uniform(0, step, size=n)).astype(np.uint64)

    def put(case, icao, samples, share=0.0):
        b.bulk.append((samples, _random_frames(rng, icao.astype(np.uint32), share), CASES.index(case)))

    special = np.array([0x000000, 0xFFFFFF, 0x7FFFFF, 0x800000], dtype=np.uint32)
    n_special = min(40, max(2, n_big // 20))
    put("seg_special", np.repeat(special, n_special), rng.integers(0, span, size=4 * n_special).astype(np.uint64))
    n_adjacent = min(64, n_single)                             # neighbours on both sides of a key byte's carry
    adjacent = np.arange(0x500100 - n_adjacent // 2, 0x500100 + (n_adjacent + 1) // 2, dtype=np.uint32)
    put("seg_adjacent", np.repeat(adjacent, 3), rng.integers(0, span, size=3 * n_adjacent).astype(np.uint64))
    base = b.next_icao["seg_single"]
    put("seg_single", base + rng.permutation(n_single).astype(np.uint32) * 3,          # gaps: never neighbours
        rng.integers(0, span, size=n_single).astype(np.uint64))
    for k, n in enumerate(edge_lengths):
        put("seg_255_256_257", np.full(n, b.next_icao["seg_255_256_257"] + k, dtype=np.uint32), evenly(n))
    put("seg_big", np.full(n_big, b.next_icao["seg_big"], dtype=np.uint32), evenly(n_big))
    weight = 1.0 / np.arange(1, n_zipf_aircraft + 1)
    who = rng.choice(n_zipf_aircraft, size=n_zipf_frames, p=weight / weight.sum())
    who[:n_zipf_aircraft] = np.arange(n_zipf_aircraft)        # everyone at least once
    put("seg_zipf", (b.next_icao["seg_zipf"] + 5 * who).astype(np.uint32),
        rng.integers(0, span, size=n_zipf_frames).astype(np.uint64), share=0.05)


def largest_window_count(icao, times):
    """The largest number of one aircraft's frames inside any 10 s window ending at one of its frames (what the pairs
    step may walk), over a list in time order."""
    order = np.lexsort((np.arange(len(icao)), icao))           # by ICAO, list order inside: the device's sort
    si, st = icao[order], times[order]
    edges = np.flatnonzero(np.concatenate([[True], si[1:] != si[:-1], [True]]))
    worst = 0
    for a, z in zip(edges[:-1], edges[1:]):
        if z - a <= worst:
            continue
        t = st[a:z]
        first_inside = np.searchsorted(t, t - WINDOW_S, side="left")
        worst = max(worst, int((np.arange(z - a) - first_inside + 1).max()))
    return worst


def hostile_traffic(oracle, seed, sps=0.5e-6, span_s=120.0, n_pairs=56, n_exact=24, n_window=17, n_per_tc=24,
                    n_single=600, n_big=2000, n_zipf_aircraft=120, n_zipf_frames=3000, edge_lengths=(255, 256, 257)):
    """The default traffic: about 11 000 frames from about 2 700 aircraft, deterministic by (seed, sps, sizes).  The
    window cases are laid out for `sps`; everything else lies in the first span_s seconds of the stream."""
    rng = np.random.default_rng(seed)
    b = _Builder(oracle, rng, sps)
    _cpr_cases(b, span_s, n_pairs, n_exact)
    _window_cases(b, n_window)
    _mix_case(b, span_s, n_per_tc)
    _segment_cases(b, span_s, n_single, n_big, n_zipf_aircraft, n_zipf_frames, edge_lengths)
    samples = np.concatenate([np.array(b.samples, dtype=np.uint64)] + [s for s, _, _ in b.bulk])
    frames = np.concatenate([np.frombuffer(b"".join(b.frames), dtype=np.uint8).reshape(-1, 14)] +
                            [f for _, f, _ in b.bulk])
    case = np.concatenate([np.array(b.case, dtype=np.int16)] + [np.full(len(s), c, dtype=np.int16) for s, _, c in b.bulk])
    order = np.argsort(samples, kind="stable")
    where = np.empty(len(order), dtype=np.int64)
    where[order] = np.arange(len(order))
    cpr_pairs = [(c, int(where[i]), int(where[j])) for c, i, j in b.cpr_pairs]
    window_pairs = [dict(p, first=int(where[p["first"]]), second=int(where[p["second"]]),
                         inside=[int(where[i]) for i in p["inside"]]) for p in b.window_pairs]
    t = Traffic(sps, samples[order], frames[order].copy(), case[order], cpr_pairs, window_pairs)
    for k in rng.integers(0, len(t), size=64):                 # the table-driven CRC is the oracle's
        assert oracle.get_adsb_crc(bytes(t.frames[k, :11])) == int.from_bytes(bytes(t.frames[k, 11:]), "big")
    assert len({int(c) for c in np.unique(t.case)}) == len(CASES)
    by_icao = {}
    for i, c in zip(t.icao.tolist(), t.case.tolist()):         # every case on ICAOs of its own
        assert by_icao.setdefault(i, c) == c, hex(i)
    assert largest_window_count(t.icao, t.times()) <= MAX_IN_WINDOW
    return t


# the small traffic of tests/golden/hostile_traffic.npz (tests/golden/make_golden.py): every case, a few frames each
GOLDEN = dict(seed=77, sps=0.5e-6, span_s=30.0, n_pairs=1, n_exact=1, n_window=1, n_per_tc=1, n_single=8, n_big=40,
              n_zipf_aircraft=5, n_zipf_frames=30, edge_lengths=(3,))


def census(oracle, traffic, sps=None):
    """Replays the traffic through the oracle alone; returns a dict:
      cases[case]       frames, aircraft, evaluations (pairs the oracle took to the CPR decode), accepted (new
                        positions), and how many evaluations reached each key of classify()
      window[region]    exact / inside / outside: [pairs, of those the oracle accepted], with fill likewise
      type_code[tc], msg_kind[kind], other_first_byte, segment_lengths {length: aircraft}, largest_window_count
    """
    sps = traffic.sps if sps is None else sps
    times = traffic.times() if sps == traffic.sps else traffic.samples.astype(np.float64) * sps
    keys = ("refused", "fold", "lat0", "lat87p", "lat87n", "one_zone", "two_zone", "quirk", "lon_wrap")
    cases = {c: dict.fromkeys(("frames", "aircraft", "evaluations", "accepted") + keys, 0) for c in CASES}
    type_code, msg_kind = [0] * 32, [0] * 3
    tracker, last = oracle.tracker(), {}                       # last[(icao, odd)] = (time, lat field, lon field)
    new_at = np.zeros(len(traffic), dtype=bool)
    for k, (fr, t, c) in enumerate(zip(traffic.frames, times.tolist(), traffic.case.tolist())):
        fb = bytes(fr)
        p = oracle.packet_new(fb)
        new, _ = tracker.update(fb, t)
        new_at[k] = new
        row = cases[CASES[c]]
        row["frames"] += 1
        type_code[p.msg_type] += 1
        msg_kind[p.msg_kind] += 1
        if p.msg_kind != 1:
            assert not new
            continue
        odd = int(p.cpr_odd)
        last[(p.icao, odd)] = (t, p.cpr_latitude, p.cpr_longitude)
        partner = last.get((p.icao, 1 - odd))
        if partner is None or abs(t - partner[0]) > WINDOW_S:
            assert not new
            continue
        even, other = (partner, (t, p.cpr_latitude, p.cpr_longitude))[::1 if odd else -1]
        got = classify(oracle, even[1], even[2], other[1], other[2], first_is_odd=not odd)
        assert new == (not got["refused"]), k                  # the census follows the oracle's own tracker
        row["evaluations"] += 1
        row["accepted"] += new
        for key in keys:
            row[key] += got[key]
    for c, n in zip(*np.unique(traffic.case[np.unique(traffic.icao, return_index=True)[1]], return_counts=True)):
        cases[CASES[c]]["aircraft"] = int(n)
    window = {r: {"exact": [0, 0], "inside": [0, 0], "outside": [0, 0], "exact_fill": [0, 0], "outside_fill": [0, 0]}
              for r in REGIONS}
    name = {"win_exact": "exact", "win_inside": "inside", "win_outside": "outside", "win_inside_fill": "exact_fill",
            "win_outside_fill": "outside_fill"}
    for p in traffic.window_pairs:
        cell = window[p["region"]][name[p["case"]]]
        cell[0] += 1
        cell[1] += bool(new_at[p["second"]])
    lengths = np.unique(traffic.icao, return_counts=True)[1]
    return {"cases": cases, "window": window, "type_code": type_code, "msg_kind": msg_kind,
            "other_first_byte": int((traffic.frames[:, 0] != 0x8D).sum()),
            "segment_lengths": {int(n): int(c) for n, c in zip(*np.unique(lengths, return_counts=True))},
            "largest_window_count": largest_window_count(traffic.icao, times), "new_positions": int(new_at.sum()),
            "frames": len(traffic), "aircraft": len(lengths)}


def check_census(c):
    """The floors of the default traffic, counted on the oracle: every named case at least 50 times (the exact
    latitudes 20), every type code 20 times, 50 window pairs exactly at the boundary of which the oracle accepts at
    least 40, and the device's 256-frames-per-window condition."""
    cases, window = c["cases"], c["window"]
    assert cases["cpr_uniform"]["evaluations"] >= 50
    for case, key in CPR_TARGET.items():
        assert cases[case][key] >= (20 if case in EXACT_LATITUDE_CASES else 50), (case, cases[case])
    assert sum(cases[k]["lon_wrap"] for k in CPR_CASES) >= 50
    total = {k: [sum(window[r][k][j] for r in REGIONS) for j in (0, 1)] for k in window[REGIONS[0]]}
    assert total["exact"][0] >= 50 and total["exact"][1] >= 40, total
    assert total["inside"][0] >= 50 and total["inside"][1] == total["inside"][0], total
    assert total["outside"][0] >= 50 and total["outside_fill"][0] >= 50, total
    assert total["exact_fill"][0] >= 50 and total["exact_fill"][1] >= 40, total
    for r in REGIONS:                                          # every stream position carries its share
        assert all(window[r][k][0] >= 15 for k in window[r]), (r, window[r])
        if r != "above_2^53":                                  # there one sample is below the times' resolution
            assert window[r]["outside"][1] == window[r]["outside_fill"][1] == 0, (r, window[r])
    assert min(c["type_code"]) >= 20, c["type_code"]
    assert min(c["msg_kind"]) >= 50 and c["other_first_byte"] >= 50
    assert cases["mix"]["frames"] >= 50
    lengths = c["segment_lengths"]
    assert lengths.get(1, 0) >= 50 and all(lengths.get(n, 0) >= 1 for n in (255, 256, 257))
    assert cases["seg_special"]["aircraft"] == 4 and cases["seg_adjacent"]["aircraft"] >= 50
    assert cases["seg_big"]["frames"] >= 0.1 * c["frames"] and cases["seg_zipf"]["aircraft"] >= 50
    assert c["largest_window_count"] <= MAX_IN_WINDOW


def census_table(c):
    """The census as text, one row per case."""
    keys = ("frames", "aircraft", "evaluations", "accepted", "refused", "fold", "lat0", "lat87p", "lat87n", "one_zone",
            "two_zone", "quirk", "lon_wrap")
    short = ("frames", "acft", "evals", "accept", "refuse", "fold", "lat0", "+87", "-87", "1zone", "2zone", "quirk",
             "wrap")
    lines = [f"{'case':17s}" + "".join(f"{s:>7s}" for s in short)]
    for case in CASES:
        lines.append(f"{case:17s}" + "".join(f"{c['cases'][case][k]:7d}" for k in keys))
    for r in REGIONS:
        lines.append(f"window {r:12s} " + "  ".join(f"{k} {v[1]}/{v[0]}" for k, v in c["window"][r].items()) +
                     "  (accepted / pairs)")
    lines.append("type codes 0-31: " + " ".join(str(x) for x in c["type_code"]))
    lines.append(f"msg_kind id / position / unknown: {c['msg_kind']}; first byte not 0x8D: {c['other_first_byte']}; "
                 f"frames {c['frames']}, aircraft {c['aircraft']}, new positions {c['new_positions']}, largest count in "
                 f"a 10 s window {c['largest_window_count']}")
    top = sorted(c["segment_lengths"].items())
    lines.append("segment lengths (length: aircraft): " + " ".join(f"{n}:{k}" for n, k in top))
    return "\n".join(lines)


if __name__ == "__main__":                                     # python -m tests.hostile_traffic [seed]: the census tables
    import sys

    from tests.oracle_binding import Oracle
    for period in SAMPLE_PERIODS:
        made = hostile_traffic(Oracle(), int(sys.argv[1]) if len(sys.argv) > 1 else 101, period)
        print(f"hostile_traffic(seed={sys.argv[1] if len(sys.argv) > 1 else 101}, sps={period!r})")
        print(census_table(census(Oracle(), made)))
