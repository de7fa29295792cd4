// adsb_commb.h -- which Comm-B register the MB field of one DF20/21 reply carries, and its values (include/adsb_hip.h,
// "Comm-B registers"): the seven candidate tests, the state they give, and the decode of the one register that passes.
// One text for the device (adsb_commb.hip) and the CPU mirror (host/adsb_commb.cpp, adsb_host_commb): every function
// here is __host__ __device__ under hipcc and plain inline C++ otherwise.  Integers only.  Built on adsb_modes.h's
// ModesBytes: MB is one 56-bit number cut from the frame's two words, every field a shift and a mask of it, so a frame
// stays in registers and no array is indexed by a variable.
#ifndef ADSB_COMMB_H
#define ADSB_COMMB_H

#include <stdint.h>

#include "../../include/adsb_hip.h"
#include "adsb_modes.h"

namespace adsbk {

constexpr uint32_t kCommbRegisters = 7;
// the header's totals as the kernels count them: the five states, then the ONE records of each register
constexpr uint32_t kCommbTallies = 5 + kCommbRegisters;

// the candidate bit of a BDS code, 0 for a code that is none of the seven
ADSB_WIRE_HD inline uint32_t commb_bit_of(uint32_t bds)
{
    if (bds == 0x10u) return ADSB_COMMB_C10;
    if (bds == 0x17u) return ADSB_COMMB_C17;
    if (bds == 0x20u || bds == 0x30u || bds == 0x40u || bds == 0x50u || bds == 0x60u) return 1u << (bds >> 4);
    return 0u;
}

// MB, bit 1 in bit 55 of v
struct CommbMb {
    uint64_t v;
    // u(a, n), n <= 32
    ADSB_WIRE_HD uint32_t u(uint32_t a, uint32_t n) const { return (uint32_t)((v >> (57u - a - n)) & ((1ull << n) - 1ull)); }
    // s(a, n): a sign bit at a, then n bits
    ADSB_WIRE_HD int32_t s(uint32_t a, uint32_t n) const { return (int32_t)u(a + 1u, n) - (int32_t)(u(a, 1) << n); }
    ADSB_WIRE_HD bool bit(uint32_t a) const { return u(a, 1) != 0u; }
    // the status rule (a; n)
    ADSB_WIRE_HD bool rule(uint32_t a, uint32_t n) const { return bit(a) || u(a, n + 1u) == 0u; }
};
ADSB_WIRE_HD inline CommbMb commb_mb(const ModesBytes &b) { return CommbMb{(b.w0 & 0xFFFFFFFFull) << 24 | b.w1 >> 40}; }

ADSB_WIRE_HD inline uint32_t commb_abs(int32_t x) { return (uint32_t)(x < 0 ? -x : x); }

ADSB_WIRE_HD inline bool commb_is_10(const CommbMb &m)
{
    const uint32_t ovc = m.u(15, 1), ver = m.u(17, 7);
    return m.u(1, 8) == 0x10u && m.u(10, 5) == 0u && ((ovc == 1u && ver >= 5u) || (ovc == 0u && ver <= 4u));
}
ADSB_WIRE_HD inline bool commb_is_17(const CommbMb &m) { return m.u(29, 28) == 0u && m.bit(7); }
ADSB_WIRE_HD inline bool commb_is_20(const CommbMb &m)
{
    bool all = m.u(1, 8) == 0x20u;
    for (uint32_t k = 0; k < 8; ++k) {
        bool ok;
        (void)modes_char(m.u(9u + 6u * k, 6), &ok);
        all = all && ok;
    }
    return all;
}
ADSB_WIRE_HD inline bool commb_is_30(const CommbMb &m) { return m.u(1, 8) == 0x30u && m.u(29, 2) != 3u && m.u(16, 7) < 48u; }
ADSB_WIRE_HD inline bool commb_is_40(const CommbMb &m)
{
    return m.rule(1, 12) && m.rule(14, 12) && m.rule(27, 12) && m.u(40, 8) == 0u && m.u(52, 2) == 0u;
}
ADSB_WIRE_HD inline bool commb_is_50(const CommbMb &m)
{
    if (!(m.rule(1, 10) && m.rule(12, 11) && m.rule(24, 10) && m.rule(35, 10) && m.rule(46, 10))) return false;
    const int32_t gs = (int32_t)m.u(25, 10), tas = (int32_t)m.u(47, 10);
    if (m.bit(1) && commb_abs(m.s(2, 9)) > 284u) return false;
    if (m.bit(24) && gs > 300) return false;
    if (m.bit(46) && tas > 250) return false;
    if (m.bit(24) && m.bit(46) && commb_abs(tas - gs) > 100u) return false;
    return true;
}
ADSB_WIRE_HD inline bool commb_is_60(const CommbMb &m)
{
    if (!(m.rule(1, 11) && m.rule(13, 10) && m.rule(24, 10) && m.rule(35, 10) && m.rule(46, 10))) return false;
    if (m.bit(13) && m.u(14, 10) > 500u) return false;
    if (m.bit(24) && m.u(25, 10) > 250u) return false;
    if (m.bit(35) && commb_abs(m.s(36, 9)) > 187u) return false;
    if (m.bit(46) && commb_abs(m.s(47, 9)) > 187u) return false;
    return true;
}

// the candidate bits of a non-zero MB
ADSB_WIRE_HD inline uint32_t commb_candidates(const CommbMb &m)
{
    return (commb_is_10(m) ? ADSB_COMMB_C10 : 0u) | (commb_is_17(m) ? ADSB_COMMB_C17 : 0u) |
           (commb_is_20(m) ? ADSB_COMMB_C20 : 0u) | (commb_is_30(m) ? ADSB_COMMB_C30 : 0u) |
           (commb_is_40(m) ? ADSB_COMMB_C40 : 0u) | (commb_is_50(m) ? ADSB_COMMB_C50 : 0u) |
           (commb_is_60(m) ? ADSB_COMMB_C60 : 0u);
}

// value k of five, held only with the status bit at `a`
#define ADSB_COMMB_VALUE(k, a, expr)          \
    do {                                      \
        if (m.bit(a)) {                       \
            r.value[k] = (int32_t)(expr);     \
            status |= 1u << (k);              \
        }                                     \
    } while (0)

// r becomes the ONE record of MB read as the register with candidate bit `c` (one bit); candidates and n_candidates
// stay as they are
ADSB_WIRE_HD inline void commb_decode(const CommbMb &m, uint32_t c, adsb_commb_rec &r)
{
    uint32_t status = 0, word = 0, bds = 0;
    r.value[0] = r.value[1] = r.value[2] = r.value[3] = r.value[4] = 0;
    if (c == ADSB_COMMB_C10) {
        bds = 0x10u;
        status = 0x3u;
        r.value[0] = (int32_t)m.u(17, 7);
        r.value[1] = (int32_t)m.u(15, 1);
        word = m.u(1, 32);
    } else if (c == ADSB_COMMB_C17) {
        bds = 0x17u;
        word = m.u(1, 28);
    } else if (c == ADSB_COMMB_C20) {
        bds = 0x20u;
    } else if (c == ADSB_COMMB_C30) {
        bds = 0x30u;
        status = 0x1Fu;
        r.value[0] = (int32_t)m.u(9, 14);
        r.value[1] = (int32_t)m.u(23, 4);
        r.value[2] = (int32_t)m.u(27, 2);
        r.value[3] = (int32_t)m.u(29, 2);
        r.value[4] = (int32_t)m.u(31, 26);
        word = m.u(1, 32);
    } else if (c == ADSB_COMMB_C40) {
        bds = 0x40u;
        ADSB_COMMB_VALUE(0, 1, 16u * m.u(2, 12));
        ADSB_COMMB_VALUE(1, 14, 16u * m.u(15, 12));
        ADSB_COMMB_VALUE(2, 27, 8000u + m.u(28, 12));
        ADSB_COMMB_VALUE(3, 48, m.u(49, 3));
        ADSB_COMMB_VALUE(4, 54, m.u(55, 2));
    } else if (c == ADSB_COMMB_C50) {
        bds = 0x50u;
        ADSB_COMMB_VALUE(0, 1, m.s(2, 9));
        ADSB_COMMB_VALUE(1, 12, (m.s(13, 10) + 2048) & 2047);
        ADSB_COMMB_VALUE(2, 24, 2u * m.u(25, 10));
        ADSB_COMMB_VALUE(3, 35, m.s(36, 9));
        ADSB_COMMB_VALUE(4, 46, 2u * m.u(47, 10));
    } else if (c == ADSB_COMMB_C60) {
        bds = 0x60u;
        ADSB_COMMB_VALUE(0, 1, (m.s(2, 10) + 2048) & 2047);
        ADSB_COMMB_VALUE(1, 13, m.u(14, 10));
        ADSB_COMMB_VALUE(2, 24, m.u(25, 10));
        ADSB_COMMB_VALUE(3, 35, 32 * m.s(36, 9));
        ADSB_COMMB_VALUE(4, 46, 32 * m.s(47, 9));
    }
    r.state = ADSB_COMMB_ONE;
    r.bds = (uint8_t)bds;
    r.status = (uint16_t)status;
    r.word = word;
}
#undef ADSB_COMMB_VALUE

// The record of one frame.  Every byte of it is written.
ADSB_WIRE_HD inline adsb_commb_rec commb_first(const ModesBytes &b)
{
    adsb_commb_rec r{};
    const uint32_t df = b[0] >> 3;
    if (df != 20u && df != 21u) return r; // ADSB_COMMB_NOT_COMMB = 0
    const CommbMb m = commb_mb(b);
    if (m.v == 0) {
        r.state = ADSB_COMMB_EMPTY;
        return r;
    }
    const uint32_t c = commb_candidates(m);
    r.candidates = (uint8_t)c;
    r.n_candidates = (uint8_t)((c & 1u) + (c >> 1 & 1u) + (c >> 2 & 1u) + (c >> 3 & 1u) + (c >> 4 & 1u) + (c >> 5 & 1u) + (c >> 6 & 1u));
    if (c == 0u) r.state = ADSB_COMMB_NONE;
    else if (c & (c - 1u)) r.state = ADSB_COMMB_AMBIGUOUS;
    else commb_decode(m, c, r);
    return r;
}

// which of the kCommbTallies totals a record counts for beside its state's: 5 + the register's place for ONE, else none
ADSB_WIRE_HD inline uint32_t commb_register_tally(const adsb_commb_rec &r)
{
    if (r.state != ADSB_COMMB_ONE) return 0xFFu;
    const uint32_t c = r.candidates;
    return 5u + ((c >> 1 & 1u) * 1u + (c >> 2 & 1u) * 2u + (c >> 3 & 1u) * 3u + (c >> 4 & 1u) * 4u + (c >> 5 & 1u) * 5u + (c >> 6 & 1u) * 6u);
}

// the header from the kCommbTallies totals of an n-frame list
ADSB_WIRE_HD inline void commb_header_of(uint64_t n, const uint64_t *t, adsb_commb_header *h)
{
    h->n = n;
    h->n_commb = n - t[ADSB_COMMB_NOT_COMMB];
    h->n_empty = t[ADSB_COMMB_EMPTY];
    h->n_none = t[ADSB_COMMB_NONE];
    h->n_one = t[ADSB_COMMB_ONE];
    h->n_ambiguous = t[ADSB_COMMB_AMBIGUOUS];
    for (uint32_t k = 0; k < kCommbRegisters; ++k) h->n_bds[k] = t[5u + k];
    h->reserved[0] = h->reserved[1] = h->reserved[2] = 0;
}

// The argument rule both entry points share (host code)
inline int commb_args_check(const adsb_frame *frames, size_t n)
{
    if (!frames && n) return ADSB_E_ARG;
    if ((uint64_t)n > 0xFFFFFFFFull) return ADSB_E_CAPACITY;
    return ADSB_OK;
}

} // namespace adsbk

#endif
