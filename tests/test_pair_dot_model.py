"""NumPy model of the odd sample's root argument in mags8_i8 (air_rs_amd/csrc/adsb_kernels.hip).

Per dword (I0, Q0, I1, Q1) the kernel has A = 2^23 + n0 (masked dot) and B = 2^23 + n0 + n1 (whole dword), both exact as
floats, and forms the odd sample's argument as fma(A, -(1 - 2^-24), B) = n1 + 0.5 + n0 * 2^-24, rounded once to f32 (to
nearest, or toward zero under MAGMODE 1).  The model evaluates that expression exactly in f64, applies either rounding,
takes the root with up to +-2 ulp of error and checks that the truncated root is floor(sqrt(n1)) for EVERY n1 an i8 sample
can produce.  (v_sqrt_f32 is good to 1 ulp; the margin found is about 90 ulp.)"""
import math

import numpy as np

N1 = np.arange(0, 32769, dtype=np.int64)              # every I^2 + Q^2 of an i8 sample
N0 = (0, 1, 2, 127, 16384, 32767, 32768)              # the even partner's sum of squares
WANT = np.array([math.isqrt(int(n)) for n in N1], dtype=np.int64)


def _exact_f64(n0):
    """B - A * (1 - 2^-24) in f64: every intermediate fits 53 bits (A * (1 - 2^-24) needs 48, the sum 40)."""
    a = np.float64(2 ** 23 + n0)
    b = (2 ** 23 + n0 + N1).astype(np.float64)
    x = b - a * np.float64(1.0 - 2.0 ** -24)
    assert (x == N1 + 0.5 + n0 * 2.0 ** -24).all()     # the identity the kernel's comment states, bit for bit
    return x


def _round_f32(x, toward_zero):
    f = x.astype(np.float32)                           # to nearest even
    if toward_zero:
        over = f.astype(np.float64) > x                # x > 0: toward zero = down
        f = np.where(over, np.nextafter(f, np.float32(0)), f).astype(np.float32)
        assert (f.astype(np.float64) <= x).all()
    return f


def _roots_pm2ulp(f):
    """sqrt of an f32 argument, correctly rounded to f32, and its neighbours up to two ulp either side"""
    r = np.sqrt(f.astype(np.float64)).astype(np.float32)
    out = [r]
    lo = hi = r
    for _ in range(2):
        lo = np.nextafter(lo, np.float32(-np.inf))
        hi = np.nextafter(hi, np.float32(np.inf))
        out += [lo, hi]
    return out


def test_odd_sample_argument_gives_floor_sqrt():
    closest = np.inf
    for n0 in N0:
        x = _exact_f64(n0)
        for toward_zero in (False, True):
            f = _round_f32(x, toward_zero)
            delta = f.astype(np.float64) - N1
            assert delta.min() >= 0.49 and delta.max() <= 0.51, (n0, toward_zero, delta.min(), delta.max())
            for r in _roots_pm2ulp(f):
                # MAGMODE 0 / 1: the converter truncates the root
                got = np.floor(r.astype(np.float64)).astype(np.int64)
                bad = np.nonzero(got != WANT)[0]
                assert bad.size == 0, (n0, toward_zero, bad[:5], got[bad[:5]], WANT[bad[:5]])
                # MAGMODE 2: root - 0.5 (one f32 subtraction), converter rounds to nearest even
                got2 = np.rint((r - np.float32(0.5)).astype(np.float64)).astype(np.int64)
                bad = np.nonzero(got2 != WANT)[0]
                assert bad.size == 0, (n0, toward_zero, bad[:5], got2[bad[:5]], WANT[bad[:5]])
            r64 = np.sqrt(f.astype(np.float64))
            closest = min(closest, float(np.abs(r64 - np.rint(r64)).min()))
    # n = k^2 - 1: k - sqrt(k^2 - 1 + d) ~ (1 - d) / 2k >= 0.498 / 362; n = k^2: sqrt(k^2 + d) - k ~ d / 2k >= 0.5 / 362
    # (k <= 181): the margin n + 0.5 has, about 90 ulp of a root near 181 (2^-16 each)
    assert closest >= 1.3e-3, closest


def test_even_sample_argument_is_exact():
    # A - (2^23 - 0.5) = n0 + 0.5 needs 17 bits: exact under either rounding
    a = (2 ** 23 + N1).astype(np.float32)
    assert (a.astype(np.int64) == 2 ** 23 + N1).all()
    e = (a.astype(np.float64) - 8388607.5)
    assert (e.astype(np.float32).astype(np.float64) == N1 + 0.5).all()


def test_multiplier_is_the_largest_float_below_one():
    m = np.float32(1.0) - np.float32(2.0 ** -24)
    assert float(m) == 1.0 - 2.0 ** -24 and m == np.nextafter(np.float32(1), np.float32(0))
    assert float.fromhex("0x1.fffffep-1") == float(m)   # the literal in mags8_i8
