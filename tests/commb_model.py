"""Independent model of the Comm-B stage (include/adsb_hip.h, "Comm-B registers"), written from the header text in plain
Python: MB as a string of 56 binary digits, so that bit a of the text is character a - 1, the seven candidate tests, the
states and the values register by register.  Calls no library entry point.  Shared by the CPU and GPU tiers, with the
comparison of a library result against it and the makers of MB fields the case lists are built with."""
import numpy as np

NOT_COMMB, EMPTY, NONE, ONE, AMBIGUOUS = range(5)
STATE_NAMES = ("NOT_COMMB", "EMPTY", "NONE", "ONE", "AMBIGUOUS")
REGISTERS = (0x10, 0x17, 0x20, 0x30, 0x40, 0x50, 0x60)          # in the order of the candidate bits
BIT = {bds: 1 << k for k, bds in enumerate(REGISTERS)}
HEADER_FIELDS = ("n", "n_commb", "n_empty", "n_none", "n_one", "n_ambiguous")
FRAME_DTYPE = np.dtype([("offset", "<u8"), ("bytes", "u1", (14,)), ("status", "u1"), ("fixed_bit", "u1")])
REC_DTYPE = np.dtype([("state", "u1"), ("bds", "u1"), ("candidates", "u1"), ("n_candidates", "u1"), ("status", "<u2"),
                      ("reserved", "<u2"), ("value", "<i4", (5,)), ("word", "<u4")])
HEADER_DTYPE = np.dtype([(k, "<u8") for k in HEADER_FIELDS] + [("n_bds", "<u8", (7,)), ("reserved", "<u8", (3,))])
LETTERS_DIGITS_SPACE = set(range(1, 27)) | set(range(48, 58)) | {32}


class MB:
    """the 56 bits, numbered from 1"""

    def __init__(self, seven_bytes):
        assert len(seven_bytes) == 7
        self.digits = "".join(f"{x:08b}" for x in bytes(seven_bytes))

    def u(self, a, n):
        assert 1 <= a and a + n - 1 <= 56
        return int(self.digits[a - 1:a - 1 + n], 2)

    def s(self, a, n):
        return self.u(a + 1, n) - (2 ** n if self.digits[a - 1] == "1" else 0)

    def bit(self, a):
        return self.digits[a - 1] == "1"

    def rule(self, a, n):
        """the status rule (a; n)"""
        return self.bit(a) or self.u(a, n + 1) == 0


def is_10(m):
    ovc, ver = m.u(15, 1), m.u(17, 7)
    return m.u(1, 8) == 0x10 and m.u(10, 5) == 0 and ((ovc == 1 and ver >= 5) or (ovc == 0 and ver <= 4))


def is_17(m):
    return m.u(29, 28) == 0 and m.bit(7)


def is_20(m):
    return m.u(1, 8) == 0x20 and all(m.u(9 + 6 * k, 6) in LETTERS_DIGITS_SPACE for k in range(8))


def is_30(m):
    return m.u(1, 8) == 0x30 and m.u(29, 2) != 3 and m.u(16, 7) < 48


def is_40(m):
    return m.rule(1, 12) and m.rule(14, 12) and m.rule(27, 12) and m.u(40, 8) == 0 and m.u(52, 2) == 0


def is_50(m):
    if not all(m.rule(a, n) for a, n in ((1, 10), (12, 11), (24, 10), (35, 10), (46, 10))):
        return False
    if m.bit(1) and abs(m.s(2, 9)) > 284:
        return False
    if m.bit(24) and m.u(25, 10) > 300:
        return False
    if m.bit(46) and m.u(47, 10) > 250:
        return False
    if m.bit(24) and m.bit(46) and abs(m.u(47, 10) - m.u(25, 10)) > 100:
        return False
    return True


def is_60(m):
    if not all(m.rule(a, n) for a, n in ((1, 11), (13, 10), (24, 10), (35, 10), (46, 10))):
        return False
    if m.bit(13) and m.u(14, 10) > 500:
        return False
    if m.bit(24) and m.u(25, 10) > 250:
        return False
    if m.bit(35) and abs(m.s(36, 9)) > 187:
        return False
    if m.bit(46) and abs(m.s(47, 9)) > 187:
        return False
    return True


TESTS = {0x10: is_10, 0x17: is_17, 0x20: is_20, 0x30: is_30, 0x40: is_40, 0x50: is_50, 0x60: is_60}


def candidates(m):
    """the registers that pass, as a list of codes in the order of the candidate bits"""
    return [bds for bds in REGISTERS if TESTS[bds](m)]


def values(m, bds):
    """(status, value[5], word) of MB read as register bds"""
    def held(fields):
        status, value = 0, [0] * 5
        for k, (a, v) in enumerate(fields):
            if m.bit(a):
                status, value[k] = status | 1 << k, v
        return status, value, 0

    if bds == 0x40:
        return held([(1, 16 * m.u(2, 12)), (14, 16 * m.u(15, 12)), (27, 8000 + m.u(28, 12)), (48, m.u(49, 3)), (54, m.u(55, 2))])
    if bds == 0x50:
        return held([(1, m.s(2, 9)), (12, m.s(13, 10) % 2048), (24, 2 * m.u(25, 10)), (35, m.s(36, 9)), (46, 2 * m.u(47, 10))])
    if bds == 0x60:
        return held([(1, m.s(2, 10) % 2048), (13, m.u(14, 10)), (24, m.u(25, 10)), (35, 32 * m.s(36, 9)), (46, 32 * m.s(47, 9))])
    if bds == 0x30:
        return 0x1F, [m.u(9, 14), m.u(23, 4), m.u(27, 2), m.u(29, 2), m.u(31, 26)], m.u(1, 32)
    if bds == 0x10:
        return 0x3, [m.u(17, 7), m.u(15, 1), 0, 0, 0], m.u(1, 32)
    if bds == 0x17:
        return 0, [0] * 5, m.u(1, 28)
    assert bds == 0x20
    return 0, [0] * 5, 0


def record(frame_bytes, as_bds=None):
    """One frame's record as a REC_DTYPE scalar's tuple.  as_bds: decode as that register, which must be a candidate
    (adsb_host_commb_as); None: the inference."""
    b = bytes(frame_bytes)
    if b[0] >> 3 not in (20, 21):
        assert as_bds is None
        return (NOT_COMMB, 0, 0, 0, 0, 0, [0] * 5, 0)
    m = MB(b[4:11])
    if m.digits == "0" * 56:
        assert as_bds is None
        return (EMPTY, 0, 0, 0, 0, 0, [0] * 5, 0)
    cand = candidates(m)
    mask = sum(BIT[c] for c in cand)
    if as_bds is not None:
        assert as_bds in cand
        cand = [as_bds]
    if len(cand) == 0:
        return (NONE, 0, mask, 0, 0, 0, [0] * 5, 0)
    if len(cand) > 1:
        return (AMBIGUOUS, 0, mask, len(cand), 0, 0, [0] * 5, 0)
    status, value, word = values(m, cand[0])
    return (ONE, cand[0], mask, bin(mask).count("1"), status, 0, value, word)


def commb(frames):
    """The whole definition over a FRAME_DTYPE array (or a list of 14-byte strings) -> dict(recs, header)."""
    if not isinstance(frames, np.ndarray):
        frames = frame_list(frames)
    recs = np.zeros(len(frames), dtype=REC_DTYPE)
    for j, row in enumerate(frames["bytes"]):
        recs[j] = record(row.tobytes())
    header = dict(n=len(frames), n_commb=int((recs["state"] != NOT_COMMB).sum()), n_empty=int((recs["state"] == EMPTY).sum()),
                  n_none=int((recs["state"] == NONE).sum()), n_one=int((recs["state"] == ONE).sum()),
                  n_ambiguous=int((recs["state"] == AMBIGUOUS).sum()),
                  n_bds=[int(((recs["state"] == ONE) & (recs["bds"] == bds)).sum()) for bds in REGISTERS], reserved=[0, 0, 0])
    return dict(recs=recs, header=header)


def header_dict(header):
    """a library header (COMMB_HEADER_DTYPE record) as the model spells it"""
    out = {k: int(header[k]) for k in HEADER_FIELDS}
    out["n_bds"] = [int(x) for x in header["n_bds"]]
    out["reserved"] = [int(x) for x in header["reserved"]]
    return out


def same(got, want, what=""):
    """A library result (recs, header) against the model's, byte for byte."""
    recs, header = got
    assert header_dict(header) == want["header"], (what, header, want["header"])
    assert len(recs) == len(want["recs"]), (what, len(recs), len(want["recs"]))
    if recs.tobytes() != want["recs"].tobytes():
        bad = [j for j in range(len(recs)) if recs[j].tobytes() != want["recs"][j].tobytes()][:4]
        raise AssertionError((what, "recs", [(j, recs[j], want["recs"][j]) for j in bad]))


# ---- frames and MB fields ------------------------------------------------------------------------------------------------
def frame_list(msgs):
    fr = np.zeros(len(msgs), dtype=FRAME_DTYPE)
    for i, msg in enumerate(msgs):
        fr["bytes"][i][:len(msg)] = np.frombuffer(bytes(msg), dtype=np.uint8)
    fr["offset"] = np.arange(len(msgs)) * 500
    fr["fixed_bit"] = 0xFF
    return fr


def frame(mb, df=20, head=b"\x00\x02\x9c", parity=b"\x12\x34\x56"):
    """A 14-byte frame of format df around the 7 bytes of mb.  The stage reads neither the head nor the parity."""
    assert len(mb) == 7 and len(head) == 3 and len(parity) == 3
    return bytes([df << 3]) + bytes(head) + bytes(mb) + bytes(parity)


def mb_of(fields, ones=()):
    """MB from {first bit: (width, value)} with a negative value in two's complement of the width, and single bits set."""
    v = 0
    for a, (n, x) in fields.items():
        assert -(1 << n >> 1) <= x < (1 << n) and a + n - 1 <= 56
        v |= (x & ((1 << n) - 1)) << (57 - a - n)
    for a in ones:
        v |= 1 << (56 - a)
    return v.to_bytes(7, "big")


def with_bit(mb, a, on=True):
    v = int.from_bytes(mb, "big")
    v = v | 1 << (56 - a) if on else v & ~(1 << (56 - a))
    return v.to_bytes(7, "big")


def mb_50(roll=None, track=None, gs=None, rate=None, tas=None):
    """BDS 5,0 from raw field values (None: status bit and field zero); each signed one as s(a, n)'s number"""
    f = {}
    for a, n, x in ((1, 10, roll), (12, 11, track), (24, 10, gs), (35, 10, rate), (46, 10, tas)):
        if x is not None:
            f[a] = (1, 1)
            f[a + 1] = (n, x)
    return mb_of(f)


def mb_60(heading=None, ias=None, mach=None, baro=None, inertial=None):
    f = {}
    for a, n, x in ((1, 11, heading), (13, 10, ias), (24, 10, mach), (35, 10, baro), (46, 10, inertial)):
        if x is not None:
            f[a] = (1, 1)
            f[a + 1] = (n, x)
    return mb_of(f)


def mb_40(mcp=None, fms=None, baro=None, modes=None, source=None):
    f = {}
    for a, n, x in ((1, 12, mcp), (14, 12, fms), (27, 12, baro), (48, 3, modes), (54, 2, source)):
        if x is not None:
            f[a] = (1, 1)
            f[a + 1] = (n, x)
    return mb_of(f)


def mb_10(version=0, ovc=0, more=0):
    """BDS 1,0; more: ORed over bits 9..56 as they are (bit 56 = 1)"""
    return (int.from_bytes(mb_of({1: (8, 0x10), 15: (1, ovc), 17: (7, version)}), "big") | more).to_bytes(7, "big")


def mb_17(bits):
    """BDS 1,7 with the listed MB bits (1..28) set"""
    return mb_of({}, ones=bits)


def mb_20(text):
    charset = "#ABCDEFGHIJKLMNOPQRSTUVWXYZ#####_###############0123456789######"
    return mb_of(dict([(1, (8, 0x20))] + [(9 + 6 * k, (6, charset.index(ch))) for k, ch in enumerate(text)]))


def mb_30(ara=0, rac=0, rat_mte=0, tti=0, tid=0):
    return mb_of({1: (8, 0x30), 9: (14, ara), 23: (4, rac), 27: (2, rat_mte), 29: (2, tti), 31: (26, tid)})
