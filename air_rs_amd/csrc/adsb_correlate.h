// adsb_correlate.h -- receptions of one transmission across receivers (include/adsb_hip.h, "Correlate"): the 112-bit
// key and its compare, the group order, the head rule and the associative combine of the per-group aggregate (counts,
// the 256-bit receiver set, the holder of the least status, the holder of the best level, first and last time).  One
// text for the device (adsb_correlate.hip, a segmented scan with this combine) and the CPU mirror
// (host/adsb_correlate.cpp, adsb_host_correlate, a walk with the same combine): every function here is
// __host__ __device__ under hipcc and plain inline C++ otherwise.  Integers only, so both sides agree to the bit.
#ifndef ADSB_CORRELATE_H
#define ADSB_CORRELATE_H

#include <stdint.h>

#include "../../include/adsb_hip.h"

#if defined(__HIPCC__)
#define ADSB_CORR_HD __host__ __device__
#else
#define ADSB_CORR_HD
#endif

namespace adsbk {

constexpr uint32_t kCorrMaxReceivers = 256;
constexpr uint16_t kCorrNoReceiver = 0xFFFFu;

// K as two words: hi = bytes 0..5 (48 bits), lo = bytes 6..13 (64 bits), both big-endian.  K = hi x 2^64 + lo.
ADSB_CORR_HD inline uint64_t corr_key_hi(const uint8_t *b)
{
    uint64_t v = 0;
    for (uint32_t k = 0; k < 6; ++k) v = (v << 8) | b[k];
    return v;
}

ADSB_CORR_HD inline uint64_t corr_key_lo(const uint8_t *b)
{
    uint64_t v = 0;
    for (uint32_t k = 6; k < 14; ++k) v = (v << 8) | b[k];
    return v;
}

// One reception as the group order sees it.
struct CorrRec {
    uint64_t t, lo, hi;
};

ADSB_CORR_HD inline bool corr_same_key(const CorrRec &a, const CorrRec &b) { return a.hi == b.hi && a.lo == b.lo; }

// Group order: (K, T, j) ascending, all unsigned.  ja / jb: the list indices.
ADSB_CORR_HD inline bool corr_before(const CorrRec &a, uint32_t ja, const CorrRec &b, uint32_t jb)
{
    if (a.hi != b.hi) return a.hi < b.hi;
    if (a.lo != b.lo) return a.lo < b.lo;
    if (a.t != b.t) return a.t < b.t;
    return ja < jb;
}

// The head rule, for a reception and its predecessor in group order (the first in group order is a head without it):
// other bytes, or a gap above the window.  t - pred.t is uint64 arithmetic: in group order it does not go below zero.
ADSB_CORR_HD inline bool corr_is_head(const CorrRec &pred, const CorrRec &r, uint32_t window)
{
    return !corr_same_key(pred, r) || r.t - pred.t > (uint64_t)window;
}

// What a run of receptions of one group adds up to.  72 bytes.
struct CorrAgg {
    uint64_t set[4];      // receivers heard
    uint64_t first_t, last_t;
    uint64_t best_sum;    // signal_sum of the best-level holder (0: none)
    uint32_t n, n_clean;
    uint16_t first_rx;    // receiver of the run's first reception
    uint16_t best_rx;     // receiver of the best-level holder; kCorrNoReceiver: no valid level in the run
    uint8_t status, fixed_bit; // of the first reception with the least status
    uint8_t head;         // the run starts a group
    uint8_t pad;
};
static_assert(sizeof(CorrAgg) == 72, "CorrAgg layout");

// The aggregate of one reception.  lv: its level record or null.
ADSB_CORR_HD inline CorrAgg corr_agg_of(uint64_t t, uint32_t receiver, const adsb_frame &f, const adsb_frame_level *lv,
                                        bool head)
{
    CorrAgg a;
    for (uint32_t k = 0; k < 4; ++k) a.set[k] = 0;
    a.set[(receiver >> 6) & 3u] = 1ull << (receiver & 63u);
    a.first_t = a.last_t = t;
    const bool valid = lv && (lv->flags & ADSB_LEVEL_VALID);
    a.best_sum = valid ? lv->signal_sum : 0;
    a.best_rx = valid ? (uint16_t)receiver : kCorrNoReceiver;
    a.n = 1;
    a.n_clean = f.status == 0 ? 1u : 0u;
    a.first_rx = (uint16_t)receiver;
    a.status = f.status;
    a.fixed_bit = f.fixed_bit;
    a.head = head ? 1 : 0;
    a.pad = 0;
    return a;
}

// a, then b, both runs of the group order with b right behind a.  A b that starts a group drops a (the segmented scan);
// otherwise ties keep a's holder, the earlier in group order.  Associative.
ADSB_CORR_HD inline CorrAgg corr_combine(const CorrAgg &a, const CorrAgg &b)
{
    if (b.head) return b;
    CorrAgg r = a;
    for (uint32_t k = 0; k < 4; ++k) r.set[k] = a.set[k] | b.set[k];
    r.last_t = b.last_t; // group order inside a group is ascending T
    r.n = a.n + b.n;
    r.n_clean = a.n_clean + b.n_clean;
    if (b.status < a.status) {
        r.status = b.status;
        r.fixed_bit = b.fixed_bit;
    }
    if (b.best_rx != kCorrNoReceiver && (a.best_rx == kCorrNoReceiver || b.best_sum > a.best_sum)) {
        r.best_rx = b.best_rx;
        r.best_sum = b.best_sum;
    }
    return r;
}

ADSB_CORR_HD inline uint32_t corr_popcount64(uint64_t v)
{
    uint32_t n = 0;
    for (; v; v &= v - 1) ++n;
    return n;
}

// The message of a whole group: g its aggregate, bytes its key, first its first entry in receptions[].
ADSB_CORR_HD inline adsb_message corr_message_of(const CorrAgg &g, const uint8_t *bytes, uint32_t first)
{
    adsb_message m;
    m.time = g.first_t;
    for (uint32_t k = 0; k < 14; ++k) m.bytes[k] = bytes[k];
    m.status = g.status;
    m.fixed_bit = g.fixed_bit;
    m.first = first;
    m.n_receptions = g.n;
    m.n_receivers = (uint16_t)(corr_popcount64(g.set[0]) + corr_popcount64(g.set[1]) + corr_popcount64(g.set[2]) +
                               corr_popcount64(g.set[3]));
    m.first_receiver = g.first_rx;
    m.best_receiver = g.best_rx;
    m.reserved = 0;
    m.n_clean = g.n_clean;
    m.reserved2 = 0;
    m.span = g.last_t - g.first_t;
    m.best_signal_sum = g.best_rx == kCorrNoReceiver ? 0 : g.best_sum;
    return m;
}

ADSB_CORR_HD inline adsb_frame corr_frame_of(const adsb_message &m)
{
    adsb_frame f;
    f.offset = m.time;
    for (uint32_t k = 0; k < 14; ++k) f.bytes[k] = m.bytes[k];
    f.status = m.status;
    f.fixed_bit = m.fixed_bit;
    return f;
}

} // namespace adsbk

#endif
