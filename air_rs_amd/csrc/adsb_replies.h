// adsb_replies.h -- the replies scan's text of one offset and of one frame (include/adsb_hip.h, "Mode S replies from
// samples"): a sample's power, the strict preamble test, the bit slicer, the decision a candidate's DF and syndrome
// give it, the lookup in known[], the frame as it is emitted, and the place of a frame in a merge of two lists.  One
// text for the device (adsb_replies.hip) and the CPU mirror (host/adsb_replies.cpp, adsb_host_replies and
// adsb_host_merge_lists): every function here is __host__ __device__ under hipcc and plain inline C++ otherwise.
// Integers only.  The powers come through a functor p(k) = power of sample k of the channel, so the device reads them
// from LDS or from the samples and the mirror from the host buffer by the same text.
#ifndef ADSB_REPLIES_H
#define ADSB_REPLIES_H

#include <stddef.h>
#include <stdint.h>

#include "../../include/adsb_hip.h"
#include "adsb_modes.h"

namespace adsbk {

constexpr uint32_t kRepliesThreads = 256; // per workgroup of replies_scan / replies_write: one run of offsets each
constexpr uint32_t kRepliesHalo = 240;    // samples a tile reads behind its last offset: 16 + 2 x 112
constexpr uint32_t kRepliesDfSpan = 26;   // samples the preamble and the five DF bits take
// offsets per thread (one word of the tile's bitmap) and per tile
constexpr uint32_t replies_run(int sample_type) { return sample_type == ADSB_SAMPLE_I8 ? 32u : 16u; }
constexpr uint32_t replies_tile(int sample_type) { return kRepliesThreads * replies_run(sample_type); }
constexpr uint32_t kRepliesMaxChannels = 1u << 20; // adsb_merge_lists_of / adsb_host_merge_lists

// what an offset comes to
constexpr uint32_t kRepliesNoPreamble = 0;
constexpr uint32_t kRepliesPreamble = 1;  // the preamble test passes and nothing more is counted: a DF that is never
                                          // kept, or a frame that does not fit the channel
constexpr uint32_t kRepliesAllCall = 2;   // kept: DF11
constexpr uint32_t kRepliesDf18 = 3;      // kept: DF18
constexpr uint32_t kRepliesAp = 4;        // kept: an address/parity frame
constexpr uint32_t kRepliesNotKnown = 5;  // an address/parity frame the filter turned away
constexpr uint32_t kRepliesParity = 6;    // DF11 / DF18 whose check failed
// per-tile words: the frames kept, then n_preamble, n_all_call, n_df18, n_address_parity, n_not_known, n_parity
constexpr uint32_t kRepliesTallies = 6;
constexpr uint32_t kRepliesTileWords = 1 + kRepliesTallies;
ADSB_WIRE_HD inline bool replies_kept(uint32_t outcome) { return outcome >= kRepliesAllCall && outcome <= kRepliesAp; }

ADSB_WIRE_HD inline uint32_t replies_power(int32_t i, int32_t q) { return (uint32_t)(i * i) + (uint32_t)(q * q); }
// sample k of a channel that starts at `iq`
template <int ST>
ADSB_WIRE_HD inline uint32_t replies_sample_power(const void *iq, uint64_t k)
{
    if (ST == ADSB_SAMPLE_I8) {
        const int8_t *s = static_cast<const int8_t *>(iq) + 2u * k;
        return replies_power(s[0], s[1]);
    }
    const int16_t *s = static_cast<const int16_t *>(iq) + 2u * k;
    return replies_power(s[0], s[1]);
}

ADSB_WIRE_HD inline uint32_t replies_min(uint32_t a, uint32_t b) { return a < b ? a : b; }
ADSB_WIRE_HD inline uint32_t replies_max(uint32_t a, uint32_t b) { return a > b ? a : b; }

// pre(i) from the sixteen powers at i: the weakest pulse above the strongest gap, strictly
ADSB_WIRE_HD inline bool replies_preamble16(const uint32_t *w)
{
    const uint32_t pulse = replies_min(replies_min(w[0], w[2]), replies_min(w[7], w[9]));
    uint32_t gap = replies_max(replies_max(w[1], w[3]), replies_max(w[4], w[5]));
    gap = replies_max(gap, replies_max(replies_max(w[6], w[8]), replies_max(w[10], w[11])));
    gap = replies_max(gap, replies_max(replies_max(w[12], w[13]), replies_max(w[14], w[15])));
    return pulse > gap;
}
template <class P>
ADSB_WIRE_HD inline bool replies_preamble(const P &p, uint64_t i)
{
    uint32_t w[16];
    for (uint32_t k = 0; k < 16; ++k) w[k] = p(i + k);
    return replies_preamble16(w);
}

// bits first .. first + n of the frame at i (n <= 64), MSB first, in the low n bits
template <class P>
ADSB_WIRE_HD inline uint64_t replies_bits(const P &p, uint64_t i, uint32_t first, uint32_t n)
{
    uint64_t v = 0;
    for (uint32_t k = first; k < first + n; ++k) v = v << 1 | (uint64_t)(p(i + 16u + 2u * k) > p(i + 17u + 2u * k));
    return v;
}
// the frame's bytes: 7 of a short frame (bytes 7..13 are 0), 14 of a long one
template <class P>
ADSB_WIRE_HD inline ModesBytes replies_slice(const P &p, uint64_t i, uint32_t n_bits)
{
    if (n_bits == 56u) return ModesBytes{replies_bits(p, i, 0, 56) << 8, 0};
    return ModesBytes{replies_bits(p, i, 0, 64), replies_bits(p, i, 64, 48) << 16};
}

// is a in known[0 .. n): ascending, distinct
ADSB_WIRE_HD inline bool replies_is_known(const uint32_t *known, uint32_t n, uint32_t a)
{
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (known[mid] < a) lo = mid + 1u;
        else hi = mid;
    }
    return lo < n && known[lo] == a;
}

// a DF the scan may keep: DF11, DF18 and the address/parity formats DF0, 4, 5, 16, 20, 21
ADSB_WIRE_HD inline bool replies_df_wanted(uint32_t df) { return (0x00350831u >> df) & 1u; }
// what a frame of a wanted DF that fits its channel comes to, from its syndrome s
ADSB_WIRE_HD inline uint32_t replies_decide(uint32_t df, uint32_t s, uint32_t flags, const uint32_t *known, uint32_t n_known)
{
    if (df == 11) return s < 128u ? kRepliesAllCall : kRepliesParity;
    if (df == 18) return s == 0u ? kRepliesDf18 : kRepliesParity;
    if ((flags & ADSB_REPLIES_AP_KNOWN) && !replies_is_known(known, n_known, s)) return kRepliesNotKnown;
    return kRepliesAp;
}

// What offset i of a channel of n_samples samples comes to, given that pre(i) holds and i + kRepliesDfSpan <= n_samples;
// *out is the frame's bytes when it is kept.
template <class P>
ADSB_WIRE_HD inline uint32_t replies_candidate(const P &p, uint64_t i, uint64_t n_samples, uint32_t flags, const uint32_t *known,
                                               uint32_t n_known, ModesBytes *out)
{
    const uint32_t df = (uint32_t)replies_bits(p, i, 0, 5);
    if (!replies_df_wanted(df)) return kRepliesPreamble;
    const uint32_t n_bits = 8u * modes_length(df);
    if (i + 16u + 2u * n_bits > n_samples) return kRepliesPreamble;
    const ModesBytes b = replies_slice(p, i, n_bits);
    *out = b;
    return replies_decide(df, modes_syndrome(b), flags, known, n_known);
}

// The syndrome of a frame is linear in its bits: S = the XOR over its set bits of x^e mod G, e the bit's place counted
// from the frame's end (S = crc24(payload) ^ parity is the whole frame as a polynomial, mod G).  r[e] = x^e mod G: what
// the device, which slices a candidate one bit per lane, folds across the wave
struct RepliesSynTable {
    uint32_t r[112];
};
constexpr RepliesSynTable replies_syn_table()
{
    RepliesSynTable t{};
    uint32_t v = 1;
    for (uint32_t e = 0; e < 112; ++e) {
        t.r[e] = v;
        v <<= 1;
        if (v & 0x1000000u) v ^= 0x1FFF409u;
    }
    return t;
}

// the frame as it is emitted: three little-endian words of an adsb_frame
struct RepliesFrameWords {
    uint64_t w[3];
};
ADSB_WIRE_HD inline uint64_t replies_bswap64(uint64_t v)
{
    v = (v & 0x00FF00FF00FF00FFull) << 8 | (v >> 8 & 0x00FF00FF00FF00FFull);
    v = (v & 0x0000FFFF0000FFFFull) << 16 | (v >> 16 & 0x0000FFFF0000FFFFull);
    return v << 32 | v >> 32;
}
ADSB_WIRE_HD inline RepliesFrameWords replies_frame(uint64_t offset, const ModesBytes &b)
{
    // bytes[0..8), then bytes[8..14), status = 0 and fixed_bit = 0xFF
    return RepliesFrameWords{{offset, replies_bswap64(b.w0), replies_bswap64(b.w1) | 0xFFull << 56}};
}

// the header from the kRepliesTallies totals and the capacity.  Every byte of it is written.
ADSB_WIRE_HD inline void replies_header_of(const uint64_t *t, uint64_t cap, adsb_replies_header *h)
{
    const uint64_t total = t[1] + t[2] + t[3];
    h->n_out = total < cap ? total : cap;
    h->total_found = total;
    h->n_preamble = t[0];
    h->n_all_call = t[1];
    h->n_df18 = t[2];
    h->n_address_parity = t[3];
    h->n_not_known = t[4];
    h->n_parity = t[5];
    h->flags = total > cap ? ADSB_FLAG_TRUNCATED : 0u;
    h->reserved = 0;
}

// tiles of one channel: every offset i with i + kRepliesDfSpan <= n_samples is some tile's
ADSB_WIRE_HD inline uint64_t replies_tiles_per_channel(uint64_t n_samples, uint32_t tile)
{
    return (n_samples - kRepliesDfSpan + 1u + tile - 1u) / tile;
}

// Merge of two per-channel-ordered lists.  Frames before offset `key` (or up to and with it) among f[0 .. n)
ADSB_WIRE_HD inline uint64_t replies_count_before(const adsb_frame *f, uint64_t n, uint64_t key, bool with_equal)
{
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (f[mid].offset < key || (with_equal && f[mid].offset == key)) lo = mid + 1u;
        else hi = mid;
    }
    return lo;
}
// the channel of list index k: prefix[0 .. n_channels] ascending, prefix[0] = 0, k < prefix[n_channels]
ADSB_WIRE_HD inline uint32_t replies_channel_of(const uint64_t *prefix, uint32_t n_channels, uint64_t k)
{
    uint32_t lo = 0, hi = n_channels; // the last channel c with prefix[c] <= k
    while (hi - lo > 1u) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (prefix[mid] <= k) lo = mid;
        else hi = mid;
    }
    return lo;
}
// where frame k of list `mine` goes: its own index plus the frames of its channel in `other` that go in front of it; on
// equal offsets list A's frame goes first, so a frame of B counts A's equal ones and a frame of A does not count B's
ADSB_WIRE_HD inline uint64_t replies_merge_place(const adsb_frame *mine, const uint64_t *prefix_mine, const adsb_frame *other,
                                                 const uint64_t *prefix_other, uint32_t n_channels, uint64_t k, bool mine_is_b)
{
    const uint32_t c = replies_channel_of(prefix_mine, n_channels, k);
    const uint64_t o0 = prefix_other[c], o1 = prefix_other[c + 1u];
    return k + o0 + replies_count_before(other + o0, o1 - o0, mine[k].offset, mine_is_b);
}

// The argument rules the device and the host entry points share (host code).  known_host: known[] can be read here.
inline int replies_args_check(const adsb_replies_cfg *cfg, const void *iq, uint32_t n_channels, size_t n_samples,
                              size_t channel_stride, const uint32_t *known, size_t n_known, bool known_host)
{
    if (!cfg || !iq || n_channels == 0 || (!known && n_known)) return ADSB_E_ARG;
    if ((cfg->flags & ~ADSB_REPLIES_AP_KNOWN) || cfg->reserved || cfg->reserved2) return ADSB_E_ARG;
    if ((uint64_t)n_known > (1ull << kModesAddressBits)) return ADSB_E_ARG;
    if (n_samples < kRepliesDfSpan) return ADSB_E_SHORT;
    if (n_channels > 1 && channel_stride < n_samples) return ADSB_E_ARG;
    if (cfg->max_frames > 0xFFFFFFFFull) return ADSB_E_CAPACITY;
    if (known_host)
        for (size_t k = 0; k < n_known; ++k)
            if (known[k] >= kModesNoAddress || (k && known[k] <= known[k - 1])) return ADSB_E_ARG;
    return ADSB_OK;
}
inline int merge_args_check(const adsb_frame *a, const uint64_t *counts_a, const adsb_frame *b, const uint64_t *counts_b,
                            uint32_t n_channels)
{
    (void)a, (void)b;
    if (!counts_a || !counts_b || n_channels == 0 || n_channels > kRepliesMaxChannels) return ADSB_E_ARG;
    return ADSB_OK;
}

} // namespace adsbk

#endif
