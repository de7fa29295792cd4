"""The frame lists the Comm-B stage is checked on (tests/test_commb_host.py on the CPU mirror, tests/test_gpu_commb.py on
the device), built with the model's MB makers.  Each case is (name, FRAME_DTYPE list, claim); the claim is what the list
is there to show, checked against the MODEL's records by claims_hold() so that a list cannot quietly stop showing it:
  ("exact", [(state, candidate mask), ...])   every frame's state and candidates
  ("has", bit) / ("gone", bit)                every frame has / lacks that candidate
  ("pairs", bit)                              frames alternate: the even ones have the candidate, the odd ones lack it
  ("values", bds, [value[5] or None, ...])    every frame is ONE with that register; its values where a list is given
  None                                        nothing but model == library"""
import numpy as np

from tests import commb_model as M

C10, C17, C20, C30, C40, C50, C60 = (M.BIT[b] for b in M.REGISTERS)

# frame, address (from the parity), register, status, value[5], word
KNOWN = (
    ("A000029C85E42F313000007047D3", 0x4243D0, 0x40, 0x07, [3008, 3008, 10200, 0, 0], 0),
    ("A000139381951536E024D4CCF6B5", 0x3C4DD2, 0x50, 0x1F, [12, 650, 438, 4, 424], 0),
    ("A00004128F39F91A7E27C46ADC21", 0x48507F, 0x60, 0x1F, [243, 252, 105, -1920, -1920], 0),
    ("A0000638FA81C10000000081A92F", 0x484CB8, 0x17, 0x00, [0, 0, 0, 0, 0],
     sum(1 << (28 - k) for k in (1, 2, 3, 4, 5, 7, 9, 16, 17, 18, 24))),
    ("A800178D10010080F50000D5893C", 0x484B00, 0x10, 0x03, [0, 0, 0, 0, 0], 0x10010080),
    ("A000083E202CC371C31DE0AA1CCF", 0x484163, 0x20, 0x00, [0, 0, 0, 0, 0], 0),
)
KNOWN_FRAMES = [bytes.fromhex(k[0]) for k in KNOWN]

# a payload of each register with every status bit set and values well inside every limit
FULL = {0x40: M.mb_40(mcp=0x555, fms=0x2AA, baro=0x333, modes=5, source=2),
        0x50: M.mb_50(roll=-100, track=-300, gs=220, rate=-7, tas=230),
        0x60: M.mb_60(heading=-400, ias=280, mach=200, baro=-60, inertial=55)}
# status bit -> (first bit, width) of the field it guards
STATUS_FIELDS = {0x40: {1: (2, 12), 14: (15, 12), 27: (28, 12)},
                 0x50: {1: (2, 10), 12: (13, 11), 24: (25, 10), 35: (36, 10), 46: (47, 10)},
                 0x60: {1: (2, 11), 13: (14, 10), 24: (25, 10), 35: (36, 10), 46: (47, 10)}}
RESERVED = {0x10: list(range(10, 15)), 0x17: list(range(29, 57)), 0x40: list(range(40, 48)) + [52, 53]}


def known_answers():
    return "known answers", M.frame_list(KNOWN_FRAMES), ("exact", [(M.ONE, M.BIT[k[2]]) for k in KNOWN])


def status_bits(bds):
    """every status bit cleared with one bit of its field left set, bit by bit"""
    msgs = []
    for a, (first, n) in STATUS_FIELDS[bds].items():
        for keep in range(first, first + n):
            mb = M.with_bit(FULL[bds], a, False)
            for x in range(first, first + n):
                mb = M.with_bit(mb, x, x == keep)
            msgs.append(M.frame(mb))
    return f"BDS {bds >> 4},0: a status bit off over a field that is not zero", M.frame_list(msgs), ("gone", M.BIT[bds])


def reserved_bits(bds):
    base = {0x10: M.mb_10(version=3, more=0x80F50000), 0x17: M.mb_17([1, 2, 7, 9, 16, 24]), 0x40: FULL[0x40]}[bds]
    assert M.TESTS[bds](M.MB(base))
    msgs = [M.frame(M.with_bit(base, a)) for a in RESERVED[bds]]
    return f"BDS {bds >> 4},{bds & 15}: every reserved bit set", M.frame_list(msgs), ("gone", M.BIT[bds])


def limits(bds):
    """the last passing and the first failing raw value of every limit, both signs where signed"""
    if bds == 0x50:
        pairs = [(M.mb_50(roll=s * 284), M.mb_50(roll=s * 285)) for s in (1, -1)]
        pairs += [(M.mb_50(gs=300), M.mb_50(gs=301)), (M.mb_50(tas=250), M.mb_50(tas=251)),
                  (M.mb_50(gs=200, tas=100), M.mb_50(gs=201, tas=100)), (M.mb_50(gs=100, tas=200), M.mb_50(gs=100, tas=201))]
    elif bds == 0x60:
        pairs = [(M.mb_60(ias=500), M.mb_60(ias=501)), (M.mb_60(mach=250), M.mb_60(mach=251))]
        pairs += [(M.mb_60(baro=s * 187), M.mb_60(baro=s * 188)) for s in (1, -1)]
        pairs += [(M.mb_60(inertial=s * 187), M.mb_60(inertial=s * 188)) for s in (1, -1)]
    elif bds == 0x30:
        pairs = [(M.mb_30(ara=0x2A80 | 47, rac=5), M.mb_30(ara=0x2A80 | 48, rac=5)), (M.mb_30(tti=2, tid=77), M.mb_30(tti=3, tid=77))]
    else:
        assert bds == 0x10
        pairs = [(M.mb_10(version=4, ovc=0), M.mb_10(version=5, ovc=0)), (M.mb_10(version=5, ovc=1), M.mb_10(version=4, ovc=1))]
    msgs = [M.frame(mb) for pair in pairs for mb in pair]
    return f"BDS {bds >> 4},0: every limit at its last passing and first failing value", M.frame_list(msgs), ("pairs", M.BIT[bds])


def extremes():
    """every field at its minimum and maximum, s = -2^n included; whether the register still passes is the model's word"""
    msgs = []
    for lo, hi, n in ((-512, 511, "roll"), (-1024, 1023, "track"), (0, 1023, "gs"), (-512, 511, "rate"), (0, 1023, "tas")):
        msgs += [M.frame(M.mb_50(**{n: lo})), M.frame(M.mb_50(**{n: hi}))]
    for lo, hi, n in ((-1024, 1023, "heading"), (0, 1023, "ias"), (0, 1023, "mach"), (-512, 511, "baro"), (-512, 511, "inertial")):
        msgs += [M.frame(M.mb_60(**{n: lo})), M.frame(M.mb_60(**{n: hi}))]
    for hi, n in ((4095, "mcp"), (4095, "fms"), (4095, "baro"), (7, "modes"), (3, "source")):
        msgs += [M.frame(M.mb_40(**{n: 0})), M.frame(M.mb_40(**{n: hi}))]
    msgs += [M.frame(M.mb_40(mcp=4095, fms=4095, baro=4095, modes=7, source=3)),
             M.frame(M.mb_50(roll=-284, track=-1024, gs=300, rate=-512, tas=250)),
             M.frame(M.mb_60(heading=-1024, ias=500, mach=250, baro=-187, inertial=-187)),
             M.frame(M.mb_30()), M.frame(M.mb_30(ara=0x3FAF, rac=15, rat_mte=3, tti=2, tid=(1 << 26) - 1)),
             M.frame(M.mb_10()), M.frame(M.mb_10(version=127, ovc=1, more=(1 << 47) | (1 << 40) | 0xFFFFFFFF)),
             M.frame(M.mb_17([7])), M.frame(M.mb_17(range(1, 29))), M.frame(M.mb_20("________")), M.frame(M.mb_20("ZZZZ9999")),
             M.frame(b"\xff" * 7), M.frame(b"\x00" * 6 + b"\x01"), M.frame(b"\x80" + b"\x00" * 6)]
    return "every field at its minimum and maximum", M.frame_list(msgs), None


def track_and_heading():
    """the raw values -1, -1024 and 1023 of the two 11-bit angles: value = raw mod 2048.  The heading frames carry an
    inertial rate of -100 as well: 5,0 reads it as a true airspeed of 1848 kt and 4,0 as reserved bits, so 6,0 stays
    the one candidate."""
    raws = (-1, -1024, 1023)
    fr50 = M.frame_list([M.frame(M.mb_50(track=x)) for x in raws])
    fr60 = M.frame_list([M.frame(M.mb_60(heading=x, inertial=-100)) for x in raws])
    return [("true track at -1, -1024, 1023", fr50, ("values", 0x50, [[0, x % 2048, 0, 0, 0] for x in raws])),
            ("magnetic heading at -1, -1024, 1023", fr60, ("values", 0x60, [[x % 2048, 0, 0, 0, -3200] for x in raws]))]


def pass_throughs():
    payloads = [m[4:11] for m in KNOWN_FRAMES]
    msgs = [M.frame(b"\x00" * 7), M.frame(b"\x00" * 7, df=21, head=b"\xff\xff\xff", parity=b"\xff\xff\xff")]
    claim = [(M.EMPTY, 0)] * 2
    for df in (0, 4, 5, 11, 16, 17, 18, 24):
        msgs += [M.frame(p, df=df) for p in payloads]
        claim += [(M.NOT_COMMB, 0)] * len(payloads)
    msgs += [M.frame(p, df=21, head=b"\xa5\x5a\xc3", parity=b"\x00\x00\x00") for p in payloads]      # DF21 is DF20
    claim += [(M.ONE, M.BIT[k[2]]) for k in KNOWN]
    return "empty MB, other formats with the same payloads, DF21", M.frame_list(msgs), ("exact", claim)


def ambiguous():
    """5,0 with 6,0 where only one status bit they share is set, and with all of them set; 1,7 with 4,0.  A payload
    with nothing but status bit 1 and its field cannot help passing 4,0 too (it is a selected altitude there), so that
    one has three candidates."""
    both = C50 | C60
    rows = [(M.mb_50(roll=37), both | C40), (M.mb_50(roll=-284), both | C40),
            (M.mb_50(gs=250), both), (M.mb_50(gs=1), both),
            (M.mb_50(rate=187), both), (M.mb_50(rate=-187), both),
            (M.mb_50(tas=187), both), (M.mb_50(tas=3), both),
            # every status bit of both: 5,0's bit 12 is the heading's last bit, 6,0's bit 13 the track's sign
            (M.mb_50(roll=-33, track=-1024 + 420, gs=215, rate=-20, tas=180), both),
            (M.mb_of({}, ones=[1, 7, 14, 20]), C17 | C40)]
    msgs = [M.frame(mb, df=20 + k % 2) for k, (mb, _) in enumerate(rows)]
    return "constructed ambiguous payloads", M.frame_list(msgs), ("exact", [(M.AMBIGUOUS, c) for _, c in rows])


def claims_hold(case):
    """the claim of a case against the model's records"""
    name, fr, claim = case
    recs = M.commb(fr)["recs"]
    if claim is None:
        return
    if claim[0] == "exact":
        assert list(zip(recs["state"].tolist(), recs["candidates"].tolist())) == claim[1], name
    elif claim[0] == "has":
        assert (recs["candidates"] & claim[1] != 0).all(), name
    elif claim[0] == "gone":
        assert len(recs) and (recs["candidates"] & claim[1] == 0).all() and (recs["state"] >= M.NONE).all(), name
    elif claim[0] == "pairs":
        assert len(recs) and (recs["candidates"][0::2] & claim[1] != 0).all() and (recs["candidates"][1::2] & claim[1] == 0).all(), name
    elif claim[0] == "values":
        assert (recs["state"] == M.ONE).all() and (recs["bds"] == claim[1]).all(), (name, recs)
        for r, v in zip(recs, claim[2]):
            assert v is None or r["value"].tolist() == v, (name, r, v)
    else:
        raise AssertionError(claim[0])


# ---- a long mixed list ---------------------------------------------------------------------------------------------------
def _random_mb(rng, sort):
    pick = lambda lo, hi: int(rng.integers(lo, hi + 1))
    some = lambda: rng.integers(0, 2, size=5).astype(bool).tolist()
    opt = lambda on, lo, hi: pick(lo, hi) if on else None
    if sort == 0:
        ovc = pick(0, 1)
        more = (pick(0, 1) << 47) | (pick(0, 1) << 40) | pick(0, (1 << 32) - 1)
        return M.mb_10(version=pick(5, 127) if ovc else pick(0, 4), ovc=ovc, more=more)
    if sort == 1:
        return M.mb_17([7] + [a for a in range(1, 29) if rng.integers(0, 3) == 0])
    if sort == 2:
        alphabet = "ABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789_"
        return M.mb_20("".join(alphabet[pick(0, len(alphabet) - 1)] for _ in range(8)))
    if sort == 3:
        return M.mb_30(ara=pick(0, 127) << 7 | pick(0, 47), rac=pick(0, 15), rat_mte=pick(0, 3), tti=pick(0, 2), tid=pick(0, (1 << 26) - 1))
    if sort == 4:
        on = some()
        return M.mb_40(opt(on[0], 0, 4095), opt(on[1], 0, 4095), opt(on[2], 0, 4095), opt(on[3], 0, 7), opt(on[4], 0, 3))
    if sort == 5:
        on = some()
        gs = opt(on[2], 0, 300)
        tas = opt(on[4], max(0, (gs or 0) - 100) if on[2] else 0, min(250, gs + 100) if on[2] else 250)
        return M.mb_50(opt(on[0], -284, 284), opt(on[1], -1024, 1023), gs, opt(on[3], -512, 511), tas)
    if sort == 6:
        on = some()
        return M.mb_60(opt(on[0], -1024, 1023), opt(on[1], 0, 500), opt(on[2], 0, 250), opt(on[3], -187, 187), opt(on[4], -187, 187))
    if sort == 7:                                                    # 5,0 with 6,0, or 1,7 with 4,0
        kind = pick(0, 4)
        if kind == 0:
            return M.mb_50(gs=pick(1, 250))
        if kind == 1:
            return M.mb_50(rate=pick(-187, 187) or 1)
        if kind == 2:
            return M.mb_50(tas=pick(1, 187))
        if kind == 3:
            return M.mb_50(roll=pick(-284, 284), track=-1024 + pick(0, 500), gs=pick(150, 250), rate=pick(-187, 187), tas=pick(150, 187))
        return M.mb_of({2: (12, pick(0, 4095)), 15: (12, pick(0, 4095))}, ones=[1, 7, 14])
    if sort == 8:
        return b"\x00" * 7
    return bytes(rng.integers(0, 256, size=7).astype(np.uint8))      # uniformly random: nearly always NONE


def random_list(n, seed):
    """n frames: built registers of all seven kinds, ambiguous ones, empty ones, frames of other formats and uniformly
    random MB, with random heads and parities (the stage reads neither)."""
    rng = np.random.default_rng(seed)
    fr = np.zeros(n, dtype=M.FRAME_DTYPE)
    b = rng.integers(0, 256, size=(n, 14)).astype(np.uint8)
    sort = rng.integers(0, 12, size=n)                               # 9, 10: random MB; 11: another format
    df = np.where(sort == 11, rng.choice([0, 4, 5, 11, 16, 17, 18, 19, 22, 24, 31], size=n), rng.choice([20, 21], size=n))
    b[:, 0] = (df << 3 | (b[:, 0] & 7)).astype(np.uint8)
    for j in np.flatnonzero(sort <= 8):
        b[j, 4:11] = np.frombuffer(_random_mb(rng, int(sort[j])), dtype=np.uint8)
    fr["bytes"], fr["offset"], fr["fixed_bit"] = b, np.arange(n) * 240, 0xFF
    return fr


def covers_everything(recs):
    """every state, every register as ONE, and an ambiguous pair are in these records"""
    assert set(recs["state"].tolist()) == {M.NOT_COMMB, M.EMPTY, M.NONE, M.ONE, M.AMBIGUOUS}
    assert set(recs["bds"][recs["state"] == M.ONE].tolist()) == set(M.REGISTERS)
    amb = recs["candidates"][recs["state"] == M.AMBIGUOUS]
    assert (amb == C50 | C60).any() and (amb == C17 | C40).any()


def all_cases():
    cases = [known_answers()] + [status_bits(b) for b in (0x40, 0x50, 0x60)] + [reserved_bits(b) for b in (0x10, 0x17, 0x40)]
    cases += [limits(b) for b in (0x50, 0x60, 0x30, 0x10)] + [extremes()] + track_and_heading() + [pass_throughs(), ambiguous()]
    cases.append(("a random list", random_list(400, 7), None))
    return cases
