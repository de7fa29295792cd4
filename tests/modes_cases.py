"""The frame lists the Mode S stage is checked on (tests/test_modes_host.py on the CPU mirror, tests/test_gpu_modes.py on
the device), built with the model's frame makers: each case is (name, FRAME_DTYPE list, known_in)."""
import numpy as np

from tests import modes_model as M

KNOWN_FRAME = bytes.fromhex("8D4840D6202CC371C32CE0576098")
A, B, C = 0x4840D6, 0xABCDEF, 0x3C6614
UNSUPPORTED_DFS = tuple(df for df in range(32) if df not in M.SUPPORTED)


def every_kind_for_every_df():
    msgs = []
    for df in M.ADDRESS_PARITY:
        msgs += [M.reply(df, A, field=0x1234 & 0x1FFF), M.reply(df, B, low3=3, b1=0xA5, b2_high=5, field=0x0AAA)]   # KNOWN, UNKNOWN
    msgs += [M.all_call(C), M.all_call(A, iid=9), M.all_call(B, iid=127), M.all_call(A, iid=128), M.all_call(B)[:6] + b"\x00"]
    for df in (17, 18):
        good = M.squitter(B + df, df=df, me=bytes(range(7)))
        msgs += [good, good[:13] + bytes([good[13] ^ 0x40])]
    msgs += [bytes([df << 3 | 5]) + KNOWN_FRAME[1:] for df in UNSUPPORTED_DFS]
    return "every kind for every DF", M.frame_list(msgs), [A]


def fields():
    """every flag, both altitude encodings, the metric bit, emergency squawks, callsigns that are and are not text"""
    f25 = M.field_of(Q=1) | 0x0A80                              # a 25 ft code
    only_c4 = M.field_of(C4=1)
    msgs = [M.reply(4, A, low3=fs, b1=0xF8 | fs, b2_high=fs, field=f25) for fs in range(8)]
    msgs += [M.reply(5, A, low3=fs, field=f) for fs, f in ((0, 0), (2, 0x1FFF & ~0x40), (5, only_c4))]
    msgs += [M.reply(0, A, low3=4, b1=7, b2_high=4, field=only_c4), M.reply(0, A, field=0), M.reply(16, A, low3=4, field=f25),
             M.reply(16, A, b1=5, field=M.field_of(M=1, Q=1, A1=1)), M.reply(4, A, field=M.field_of(A1=1)),      # C = 0: none
             M.reply(20, A, field=M.field_of(C1=1, C2=1, C4=1, B4=1)),                                          # c = 5 <-> 7
             M.reply(20, A, low3=1, field=f25, rest=M.callsign_mb("KLM1023_")),
             M.reply(21, A, low3=4, field=0x0AAA, rest=M.callsign_mb("AB#DEFGH")),
             M.reply(21, A, field=0x1555, rest=bytes([0x21]) + M.callsign_mb("ABCDEFGH")[1:]),
             M.reply(20, A, field=only_c4, rest=M.callsign_mb("ZZZZ9999")), M.reply(24, A), M.reply(31, A, low3=7)]
    for code in (7700, 7600, 7500, 1200, 7777, 1):
        digits = [code // 1000, code // 100 % 10, code // 10 % 10, code % 10]
        bits = {l + w: d >> s & 1 for l, d in zip("ABCD", digits) for w, s in (("4", 2), ("2", 1), ("1", 0))}
        msgs.append(M.reply(5, A, field=M.field_of(**bits)))
    return "fields", M.frame_list(msgs), [A]


def bit_flips():
    df11, df17 = M.all_call(A), KNOWN_FRAME
    msgs = [bytes(df11[k] ^ (0x80 >> bit if k == byte else 0) for k in range(7)) for byte in range(7) for bit in range(8)]
    msgs += [bytes(df17[k] ^ (0x80 >> bit if k == byte else 0) for k in range(14)) for byte in range(14) for bit in range(8)]
    assert len(msgs) == 56 + 112
    return "every single-bit flip of a DF11 and a DF17 frame", M.frame_list(msgs), [A]


def iids(known):
    msgs = [M.all_call(A, iid=i) for i in range(1, 128)]
    return f"DF11 with iid 1..127, address {'known' if known else 'unknown'}", M.frame_list(msgs), [A] if known else []


def self_between():
    msgs = [M.reply(4, A), M.all_call(A), M.reply(4, A), M.reply(5, B), M.squitter(B), M.reply(5, B), M.all_call(B, iid=3)]
    return "the same address before and after its SELF frame", M.frame_list(msgs), []


def edge_addresses():
    msgs = [M.reply(4, 0), M.reply(20, 0xFFFFFF), M.squitter(0), M.squitter(0xFFFFFF, df=18), M.reply(4, 0),
            M.reply(20, 0xFFFFFF), M.all_call(0xFFFFFF, iid=1), M.all_call(0)]
    return "addresses 000000 and FFFFFF", M.frame_list(msgs), []


def duplicates():
    msgs = [M.squitter(A), M.squitter(A), M.all_call(A), M.reply(0, A), M.squitter(A), M.squitter(B), M.squitter(B)]
    return "duplicate SELF frames", M.frame_list(msgs), [B]


def known_in_sets():
    msgs = [M.reply(4, A), M.squitter(B), M.reply(5, C), M.all_call(C), M.reply(5, C), M.reply(21, B)]
    fr = M.frame_list(msgs)
    return [("known_in empty", fr, []), ("known_in of one", fr, [C]), ("known_in holds list addresses", fr, sorted([A, B, C])),
            ("known_in beside the list", fr, [1, 2, 0xFFFFFE]), ("no frames", fr[:0], [A]), ("nothing at all", fr[:0], [])]


def random_list(n, seed, n_addresses=24):
    """n frames of every sort over a small pool of addresses -> (FRAME_DTYPE list, the pool ascending)."""
    rng = np.random.default_rng(seed)
    pool = np.unique(rng.integers(0, 1 << 24, size=n_addresses)).astype(np.uint32)
    sort = rng.integers(0, 10, size=n)
    b = rng.integers(0, 256, size=(n, 14)).astype(np.uint8)
    df = np.select([sort == 0, sort == 1, sort == 2, sort == 3, sort == 4, sort == 5, sort == 6, sort == 8],
                   [17, 11, 11, rng.choice([0, 4, 5], size=n), rng.choice([16, 20, 21, 24, 27, 31], size=n),
                    rng.choice([4, 5, 20, 21], size=n), rng.choice([11, 17], size=n), 18],
                   default=b[:, 0] >> 3).astype(np.uint8)
    b[:, 0] = df << 3 | (b[:, 0] & 7)
    addr = pool[rng.integers(0, len(pool), size=n)]
    addr = np.where(sort == 5, rng.integers(0, 1 << 24, size=n), addr).astype(np.uint32)
    has_aa = np.isin(sort, (0, 1, 2, 6, 8))
    for k, shift in ((1, 16), (2, 8), (3, 0)):
        b[has_aa, k] = (addr[has_aa] >> shift) & 0xFF
    bds = np.isin(df, (20, 21)) & (rng.integers(0, 2, size=n) == 1) & (sort != 7)
    b[bds, 4] = 0x20
    text = bds & (rng.integers(0, 2, size=n) == 1)
    b[text, 5:11] = np.frombuffer(M.callsign_mb("TEST123_")[1:], dtype=np.uint8)
    word = np.select([np.isin(sort, (3, 4, 5)), sort == 2], [addr, rng.integers(1, 128, size=n)], default=0).astype(np.uint32)
    made = sort != 7                                                 # sort 7 stays random bytes, the tail of a short DF too
    short = made & (df < 16)
    long_ = made & (df >= 16)
    for rows, k in ((short, 4), (long_, 11)):
        p = M.crc24_many(b[rows, :k]) ^ word[rows]
        b[rows, k], b[rows, k + 1], b[rows, k + 2] = p >> 16, (p >> 8) & 0xFF, p & 0xFF
    b[short, 7:] = 0
    hit = np.flatnonzero(sort == 6)                                  # a self-checking frame with one bit flipped
    bit = rng.integers(8, 56, size=len(hit))                         # (not in the DF: the frame stays self-checking)
    b[hit, bit // 8] ^= (0x80 >> (bit % 8)).astype(np.uint8)
    fr = np.zeros(n, dtype=M.FRAME_DTYPE)
    fr["bytes"], fr["offset"], fr["fixed_bit"] = b, np.arange(n) * 240, 0xFF
    return fr, pool


def all_cases():
    cases = [every_kind_for_every_df(), fields(), bit_flips(), iids(True), iids(False), self_between(), edge_addresses(),
             duplicates()] + known_in_sets()
    fr, pool = random_list(300, 7)
    cases.append(("a random list", fr, pool[::2].tolist()))
    return cases
