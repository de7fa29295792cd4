// adsb_wire_in.h -- one mark of a Beast binary or AVR text stream taken apart again (include/adsb_hip.h, "Wire input"):
// type -> length, the reader of one Beast mark and of one AVR candidate, the frame's offset from its timestamp, the
// level record's sum from the signal byte, and the filters.  One text for the device (adsb_wire_in.hip, where `b` is a
// workgroup's span of the stream in LDS) and the CPU mirror (host/adsb_wire_in.cpp, adsb_host_wire_parse, where `b` is
// the stream): every function here is __host__ __device__ under hipcc and plain inline C++ otherwise.  Integers only,
// and nothing is kept in an indexed array (the 21 payload bytes travel as three words), so the device needs no scratch.
#ifndef ADSB_WIRE_IN_H
#define ADSB_WIRE_IN_H

#include <stdint.h>

#include "../../include/adsb_hip.h"
#include "adsb_synth.h"
#include "adsb_wire.h"

namespace adsbk {

constexpr uint32_t kWireInHalo = 43;     // a mark at m reads at most b[m + 1 .. m + 43]: the type byte and 21 doubled bytes
constexpr uint32_t kWireInMinBytes = 23; // the shortest long frame (Beast; an AVR line has 30 or more)
constexpr uint32_t kWireInMinShortBytes = 16; // the shortest short frame, in both formats: 1A '2' + 14, '*' + 14 digits + ';'
constexpr uint32_t kWireInMaxStreams = 256;

// what a mark turned out to be
constexpr uint32_t kWinUnknown = 0;    // Beast: a type byte other than '1', '2', '3'
constexpr uint32_t kWinCut = 1;        // another mark (Beast) or a byte that does not belong (AVR) inside it
constexpr uint32_t kWinIncomplete = 2; // it needs a byte at or past the end of its stream
constexpr uint32_t kWinOther = 3;      // complete, but no long message: counted, not emitted
constexpr uint32_t kWinLong = 4;       // complete with 14 message bytes
constexpr uint32_t kWinShort = 5;      // complete with 7 message bytes: emitted with ADSB_WIRE_IN_SHORT, else counted as other

struct WireInMark {
    uint32_t state;  // kWin*
    uint32_t end;    // where reading stopped (complete: the exclusive end of the frame's bytes), a position like the mark's
    uint32_t kind;   // the type byte ('3', ...) or the lead byte ('*', '@')
    uint32_t signal; // kWinLong / kWinShort, Beast: the signal byte; else 0
    uint64_t ticks;  // kWinLong / kWinShort: the 48-bit timestamp; 0 for a plain '*' line
    uint64_t hi, lo; // kWinLong: message bytes 0..5 (the low 48 bits of hi) and 6..13, big-endian; kWinShort: 0..5 and
                     // byte 6 in the top byte of lo, the rest of lo 0
};

// a frame that is emitted when it passes the filters
ADSB_WIRE_HD inline bool wire_in_emits(uint32_t filter, const WireInMark &r)
{
    return r.state == kWinLong || (r.state == kWinShort && (filter & ADSB_WIRE_IN_SHORT));
}

// frames that can exist in n_bytes bytes: what max_frames = 0 means
ADSB_WIRE_HD inline uint64_t wire_in_most(uint32_t filter, uint64_t n_bytes)
{
    return n_bytes / ((filter & ADSB_WIRE_IN_SHORT) ? kWireInMinShortBytes : kWireInMinBytes);
}

ADSB_WIRE_HD inline bool wire_in_cfg_ok(const adsb_wire_in_cfg *cfg)
{
    if (!cfg || cfg->format > ADSB_WIRE_AVR_MLAT || cfg->tick_bias > kWireTickMask) return false;
    return !cfg->levels || cfg->sample_type == ADSB_SAMPLE_I8 || cfg->sample_type == ADSB_SAMPLE_I16;
}

// message bytes after the 6 timestamp bytes and the signal byte; 0: an unknown type
ADSB_WIRE_HD inline uint32_t wire_in_type_length(uint32_t type)
{
    return type == '3' ? 14u : type == '2' ? 7u : type == '1' ? 2u : 0u;
}

// The Beast mark at b[m], m + 1 < limit (its type byte exists: that is part of what makes b[m] a mark).  Reads b[m + 1]
// and then b[p] only for m + 2 <= p < min(limit, m + 44).
ADSB_WIRE_HD inline WireInMark wire_in_read_beast(const uint8_t *b, uint32_t m, uint32_t limit)
{
    WireInMark r{};
    r.kind = b[m + 1];
    r.end = m + 2;
    const uint32_t len = wire_in_type_length(r.kind);
    if (!len) return r; // kWinUnknown
    uint64_t a2 = 0, a1 = 0, a0 = 0; // the bytes so far as one big-endian number
    uint32_t p = m + 2;
    for (uint32_t k = 0; k < 7 + len; ++k) {
        r.end = p;
        r.state = kWinIncomplete;
        if (p >= limit) return r;
        const uint32_t v = b[p++];
        if (v == 0x1Au) {
            if (p >= limit) return r; // the partner of a final 0x1A
            r.state = kWinCut;
            if (b[p] != 0x1Au) return r; // b[p - 1] is the next mark
            ++p;
        }
        a2 = (a2 << 8) | (a1 >> 56);
        a1 = (a1 << 8) | (a0 >> 56);
        a0 = (a0 << 8) | v;
    }
    r.end = p;
    r.state = kWinOther;
    if (len == 7) { // 14 bytes: the timestamp is the low 48 bits of a1, then the signal byte and the message in a0
        r.state = kWinShort;
        r.ticks = a1 & kWireTickMask;
        r.signal = (uint32_t)(a0 >> 56);
        r.hi = (a0 >> 8) & kWireTickMask;
        r.lo = (a0 & 0xFFull) << 56;
        return r;
    }
    if (len != 14) return r;
    r.state = kWinLong;
    r.ticks = ((a2 << 8) | (a1 >> 56)) & kWireTickMask; // bytes 0..5 of 21
    r.signal = (uint32_t)(a1 >> 48) & 0xFFu;            // byte 6
    r.hi = a1 & kWireTickMask;                          // bytes 7..12
    r.lo = a0;                                          // bytes 13..20
    return r;
}

// value of a hex digit in either case, or 16
ADSB_WIRE_HD inline uint32_t wire_in_hex(uint32_t c)
{
    if (c - '0' < 10u) return c - '0';
    const uint32_t l = (c | 0x20u) - 'a';
    return l < 6u ? l + 10u : 16u;
}

// The AVR candidate at b[p] ('*' or '@'), p < limit.  Reads b[q] only for p < q < min(limit, p + 43).
ADSB_WIRE_HD inline WireInMark wire_in_read_avr(const uint8_t *b, uint32_t p, uint32_t limit)
{
    WireInMark r{};
    r.kind = b[p];
    const bool stamped = r.kind == '@';
    uint64_t a2 = 0, a1 = 0, a0 = 0;
    uint32_t h = 0, q = p + 1;
    while (h < 41 && q < limit) {
        const uint32_t d = wire_in_hex(b[q]);
        if (d > 15u) break;
        a2 = (a2 << 4) | (a1 >> 60);
        a1 = (a1 << 4) | (a0 >> 60);
        a0 = (a0 << 4) | d;
        ++h;
        ++q;
    }
    r.end = q;
    r.state = kWinCut;
    if (h < 41 && q < limit) {
        if (b[q] != ';') return r;
        if (h == (stamped ? 40u : 28u)) {
            r.end = q + 1;
            r.state = kWinLong;
            r.ticks = stamped ? ((a2 << 16) | (a1 >> 48)) & kWireTickMask : 0ull; // digits 0..11 of 40
            r.hi = a1 & kWireTickMask;                                             // the last 28 digits
            r.lo = a0;
        } else if (h == (stamped ? 26u : 14u)) {
            r.end = q + 1;
            r.state = kWinShort;
            r.ticks = stamped ? ((a1 << 8) | (a0 >> 56)) & kWireTickMask : 0ull; // digits 0..11 of 26
            r.hi = (a0 >> 8) & kWireTickMask;                                     // the last 14 digits
            r.lo = (a0 & 0xFFull) << 56;
        } else if (h == (stamped ? 16u : 4u)) {
            r.end = q + 1;
            r.state = kWinOther;
        }
        return r;
    }
    if (q == limit && h <= (stamped ? 40u : 28u)) r.state = kWinIncomplete; // the digits reach the end of the stream
    return r;
}

// the exact inverse of wire_ticks for offsets below 2^48 / 6
ADSB_WIRE_HD inline uint64_t wire_in_offset(uint64_t ticks, uint64_t tick_bias)
{
    return ((ticks - tick_bias) & kWireTickMask) / 6ull;
}

// The smallest signal_sum whose wire_signal_byte is s: ceil((2s-1)^2 116 FS / (4 255^2)); 1 for s = 1, 0 for s = 0.  The
// largest numerator is 509^2 x 116 x 2^31, about 6.5e16.
ADSB_WIRE_HD inline uint64_t wire_in_signal_sum(uint32_t s, int sample_type)
{
    if (s < 2u) return s;
    const uint64_t unit = 116ull * (sample_type == ADSB_SAMPLE_I8 ? 32768ull : 2147483648ull);
    const uint64_t c = 2ull * s - 1ull, den = 4ull * 255ull * 255ull;
    return (c * c * unit + den - 1ull) / den;
}

ADSB_WIRE_HD inline adsb_frame_level wire_in_level(uint32_t s, int sample_type)
{
    adsb_frame_level lv{};
    if (s) {
        lv.signal_sum = wire_in_signal_sum(s, sample_type);
        lv.flags = ADSB_LEVEL_VALID;
    }
    return lv;
}

// message byte k (0..13) of a long or short mark (short: 0 from byte 7 on)
ADSB_WIRE_HD inline uint8_t wire_in_byte(const WireInMark &r, uint32_t k)
{
    return (uint8_t)(k < 6 ? r.hi >> (40u - 8u * k) : r.lo >> (56u - 8u * (k - 6u)));
}

// CRC-24 of the first 4 bytes (a short frame's payload), the shift form of adsb_synth::crc24_11
ADSB_WIRE_HD inline uint32_t wire_in_crc24_4(const uint8_t *d)
{
    uint32_t r = 0;
    for (int b = 0; b < 4; ++b) {
        r ^= (uint32_t)d[b] << 16;
        for (int i = 0; i < 8; ++i) {
            r <<= 1;
            if (r & 0x1000000u) r ^= 0x1FFF409u;
        }
    }
    return r & 0xFFFFFFu;
}

// cfg.filter on a long or short mark: true = keep.  The filters are literal: a short frame is never DF17, and an
// address/parity reply (DF0/4/5/16/20/21) never has a zero syndrome -- adsb_modes_of is the check for those.
ADSB_WIRE_HD inline bool wire_in_keep(uint32_t filter, const WireInMark &r)
{
    uint8_t d[14];
    for (uint32_t k = 0; k < 14; ++k) d[k] = wire_in_byte(r, k);
    if (r.state == kWinShort) {
        if (filter & ADSB_WIRE_IN_DF17) return false;
        if (filter & ADSB_WIRE_IN_CRC) {
            const uint32_t sent = (uint32_t)d[4] << 16 | (uint32_t)d[5] << 8 | d[6];
            if (wire_in_crc24_4(d) ^ sent) return false;
        }
        return true;
    }
    if ((filter & ADSB_WIRE_IN_DF17) && (d[0] >> 3) != 17u) return false;
    if (filter & ADSB_WIRE_IN_CRC) {
        const uint32_t sent = (uint32_t)d[11] << 16 | (uint32_t)d[12] << 8 | d[13];
        if (adsb_synth::crc24_11(d) ^ sent) return false;
    }
    return true;
}

ADSB_WIRE_HD inline adsb_frame wire_in_frame(const WireInMark &r, uint64_t tick_bias)
{
    adsb_frame f{};
    f.offset = wire_in_offset(r.ticks, tick_bias);
    for (uint32_t k = 0; k < 14; ++k) f.bytes[k] = wire_in_byte(r, k);
    f.status = 0;
    f.fixed_bit = 0xFF;
    return f;
}

// pos: the mark's position inside its own stream
ADSB_WIRE_HD inline adsb_wire_rx wire_in_rx(const WireInMark &r, uint32_t pos, uint32_t receiver)
{
    adsb_wire_rx x{};
    x.ticks = r.ticks;
    x.pos = pos;
    x.signal = (uint8_t)r.signal;
    x.kind = (uint8_t)r.kind;
    x.receiver = (uint16_t)receiver;
    return x;
}

// one mark in either format (is_beast: b[m] is a mark by the parity rule; else b[m] is '*' or '@')
ADSB_WIRE_HD inline WireInMark wire_in_read(bool is_beast, const uint8_t *b, uint32_t m, uint32_t limit)
{
    return is_beast ? wire_in_read_beast(b, m, limit) : wire_in_read_avr(b, m, limit);
}

// The header's counters as one mark changes them.  kept: the frame is emitted (wire_in_emits) and passed the filters.
struct WireInTally {
    uint32_t marks, cut, unknown, other, rejected, kept;
};
ADSB_WIRE_HD inline bool wire_in_count(const WireInMark &r, uint32_t filter, WireInTally *t)
{
    t->marks += 1;
    t->cut += r.state == kWinCut;
    t->unknown += r.state == kWinUnknown;
    const bool emits = wire_in_emits(filter, r);
    t->other += r.state == kWinOther || (r.state == kWinShort && !emits);
    if (!emits) return false;
    const bool keep = wire_in_keep(filter, r);
    t->rejected += !keep;
    t->kept += keep;
    return keep;
}

// Beast: where the carried tail of a stream of N bytes starts when no mark is incomplete.  run = the number of 0x1A
// bytes the stream ends with.  A complete frame that ends inside that run has taken an even number of its bytes (it
// reads them in pairs from the run's first byte, which comes after its type byte or a plain payload byte), so the bytes
// left over have the run's parity: the last one is carried when that is odd.
ADSB_WIRE_HD inline uint32_t wire_in_tail(uint32_t N, uint32_t run) { return N - (run & 1u); }

} // namespace adsbk

#endif
