"""The edge lists of correlate, shared by the CPU tier (the mirror against the model) and the GPU tier (the device
against the model).  Every case is (name, frames, counts, window, sample_base or None, levels or None); none depends on
the kernels' workgroup size (tests/test_gpu_correlate.py adds those)."""
import numpy as np

from tests import correlate_model as M

KNOWN = bytes.fromhex("8D4840D6202CC371C32CE0576098")
OTHER = bytes.fromhex("8D40621D58C382D690C8AC2863A7")


def _flip(b, byte, bit):
    out = bytearray(b)
    out[byte] ^= 1 << bit
    return bytes(out)


def _row(t, b=KNOWN, status=0, fixed=0xFF, sig=0, flags=0):
    return (t, b, status, fixed, sig, flags)


def chain_cases():
    """Equal bytes with gaps exactly window (joins) and window + 1 (splits); window 0; window 2^32 - 1; a chain whose
    span exceeds the window many times over."""
    out = []
    for w in (7, 0, (1 << 32) - 1):
        t, rows = 1000, []
        for gap in (w, w, w + 1, w, w + 1, w + 1, w):       # groups of 3, 2, 1, 2
            rows.append(t)
            t += gap
        rows.append(t)
        per = [[_row(x) for x in rows[0::2]], [_row(x) for x in rows[1::2]]]
        fr, counts = M.build(per)
        out.append((f"chain gaps w={w}", fr, counts, w, None, None))
    w = 5
    per = [[_row(100 + 3 * w * k + r * w) for k in range(40)] for r in range(3)]   # gaps of w: one chain of 120, span 119 w
    fr, counts = M.build(per)
    out.append(("long chain", fr, counts, w, None, None))
    per = [[_row(100 + 3 * (w + 1) * k + r * (w + 1)) for k in range(40)] for r in range(3)]  # gaps of w + 1: 120 groups
    fr, counts = M.build(per)
    out.append(("no chain", fr, counts, w, None, None))
    return out


def key_cases():
    """All 112 bits take part, unsigned: pairs that differ in bit 0 of byte 13, in bit 7 of byte 0, across the 64 / 48
    bit split, 0x7F against 0x80 -- all at equal times, so only the bytes order the messages."""
    base = bytes([0x40] * 14)
    keys = [base, _flip(base, 13, 0), _flip(base, 0, 7), _flip(base, 5, 0), _flip(base, 6, 7), _flip(base, 6, 0),
            bytes([0x7F] * 14), bytes([0x80] * 14), bytes([0x7F] + [0] * 13), bytes([0x80] + [0] * 13),
            bytes([0] * 6 + [0x7F] + [0] * 7), bytes([0] * 6 + [0x80] + [0] * 7), bytes([0] * 14), bytes([0xFF] * 14),
            bytes([0] * 5 + [1] + [0] * 8), bytes([0] * 6 + [0xFF] * 8)]
    assert len(set(keys)) == len(keys)
    rng = np.random.default_rng(5)
    per = [[_row(500, keys[k]) for k in rng.permutation(len(keys))] for _ in range(3)]
    fr, counts = M.build(per)
    return [("key width", fr, counts, 0, None, None)]


def time_cases():
    """T above 2^32 and above 2^63; offsets ascending per receiver while T interleaves across receivers; equal T on
    different receivers."""
    out = []
    base = [1 << 33, (1 << 63) + 5, 0, (1 << 33) - 40]
    per = [[_row(10), _row(50, OTHER), _row(3000)],
           [_row(7), _row(20, OTHER)],
           [_row((1 << 33) + 10), _row((1 << 33) + 52, OTHER), _row((1 << 63) + 12), _row((1 << 63) + 26, OTHER)],
           [_row(50), _row(90, OTHER), _row(3040)]]
    fr, counts = M.build(per)
    for w in (0, 2, 40):
        out.append((f"time width w={w}", fr, counts, w, base, None))
    # interleaved: receiver r's clock starts 7 r samples late, the same transmissions every 100 samples
    per = [[_row(100 * k, KNOWN if k % 2 else OTHER) for k in range(12)] for r in range(4)]
    fr, counts = M.build(per)
    out.append(("interleave", fr, counts, 25, [7 * r for r in range(4)], None))
    # equal T everywhere: first_receiver is the lowest list index
    per = [[_row(400 - 100 * r, status=1, fixed=r)] for r in range(4)]
    fr, counts = M.build(per)
    out.append(("equal T", fr, counts, 0, [100 * r for r in range(4)], None))
    return out


def receiver_cases():
    out = []
    per = [[_row(1000 + (r * 37) % 50)] for r in range(256)]
    fr, counts = M.build(per)
    out.append(("256 receivers", fr, counts, 50, None, None))
    per = [[_row(10), _row(12), _row(500)], [_row(11)]]                    # receiver 0 twice in the first group
    fr, counts = M.build(per)
    out.append(("one receiver twice", fr, counts, 2, None, None))
    per = [[], [], [_row(5), _row(90, OTHER)], [], [], [_row(6), _row(91, OTHER)], [_row(7)], [], []]
    fr, counts = M.build(per)
    out.append(("empty receivers", fr, counts, 3, [0, 9, 0, 9, 9, 0, 0, 9, 9], None))
    per = [[_row(5)]]
    fr, counts = M.build(per)
    out.append(("one frame", fr, counts, 3, None, None))
    return out


def status_level_cases():
    V = M.LEVEL_VALID
    per = [
        # group A (t = 100..104): all status 1, different fixed_bit; levels tie at 700 between receivers 0 and 2
        # group B (t = 300..): mixed, the clean reception is not the earliest; only some levels valid
        # group C (t = 600..): no level valid
        # group D (t = 900): a valid level of signal_sum 0
        [_row(100, status=1, fixed=11, sig=700, flags=V), _row(302, status=1, fixed=3, sig=900, flags=0),
         _row(600, sig=5, flags=0), _row(900, sig=0, flags=V)],
        [_row(101, status=1, fixed=22, sig=650, flags=V), _row(303, status=0, sig=100, flags=V), _row(601, status=1, fixed=80)],
        [_row(102, status=1, fixed=33, sig=700, flags=V), _row(301, status=1, fixed=4, sig=50, flags=V),
         _row(304, status=0, sig=100, flags=V), _row(901, sig=0, flags=0)],
    ]
    fr, counts, lv = M.build(per, levels=True)
    return [("status and levels", fr, counts, 10, None, lv), ("status, no levels", fr, counts, 10, None, None)]


def random_cases():
    out = []
    for n, seed in ((0, 1), (1, 2), (2, 3), (97, 4), (400, 5)):
        fr, counts, lv = M.random_list(n, 5, seed)
        out.append((f"random n={n}", fr, counts, 40, [3 * r for r in range(5)], lv))
        out.append((f"random n={n}, no levels", fr, counts, 40, None, None))
    return out


def all_cases():
    return (chain_cases() + key_cases() + time_cases() + receiver_cases() + status_level_cases() + random_cases())
