// adsb_modes.h -- one Mode S frame's address and surveillance fields (include/adsb_hip.h, "Mode S replies"): the frame's
// length and syndrome, the kind its format and syndrome give it before the known set is asked, the AC and ID fields
// (25 ft and Gillham altitudes, the squawk), the flags from FS / VS, the BDS 2,0 callsign, and the rule by which an
// address counts as known at a list index.  One text for the device (adsb_modes.hip) and the CPU mirror
// (host/adsb_modes.cpp, adsb_host_modes): every function here is __host__ __device__ under hipcc and plain inline C++
// otherwise.  Integers only; the CRC is the shift form, so nothing here needs a table or LDS.
#ifndef ADSB_MODES_H
#define ADSB_MODES_H

#include <stdint.h>

#include "../../include/adsb_hip.h"
#include "adsb_wire.h"

namespace adsbk {

constexpr uint32_t kModesMaxReceivers = 256;
constexpr uint32_t kModesAddressBits = 24;
constexpr uint32_t kModesNoAddress = 1u << kModesAddressBits; // the sort key of a frame that teaches no address
constexpr uint32_t kModesKeyBits = kModesAddressBits + 1;

// The 14 frame bytes as two big-endian words (bytes 0..7, bytes 8..13 in the top of w1): what the functions below read a
// byte from by a shift, so that no array is indexed by a variable and the device keeps a frame in registers
struct ModesBytes {
    uint64_t w0, w1;
    ADSB_WIRE_HD uint32_t operator[](uint32_t k) const
    {
        return (uint32_t)((k < 8u ? w0 >> (56u - 8u * k) : w1 >> (56u - 8u * (k - 8u))) & 0xFFu);
    }
};
ADSB_WIRE_HD inline ModesBytes modes_bytes(const uint8_t *b)
{
    ModesBytes x{0, 0};
    for (uint32_t k = 0; k < 8; ++k) x.w0 = x.w0 << 8 | b[k];
    for (uint32_t k = 8; k < 14; ++k) x.w1 = x.w1 << 8 | b[k];
    x.w1 <<= 16;
    return x;
}

// Mode-S CRC-24 (generator 0x1FFF409) of d[0..len), the shift form of adsb_synth::crc24_11
ADSB_WIRE_HD inline uint32_t modes_crc24(const ModesBytes &d, uint32_t len)
{
    uint32_t r = 0;
    for (uint32_t b = 0; b < len; ++b) {
        r ^= d[b] << 16;
        for (int i = 0; i < 8; ++i) {
            r <<= 1;
            if (r & 0x1000000u) r ^= 0x1FFF409u;
        }
    }
    return r & 0xFFFFFFu;
}

// bytes of a frame with this DF
ADSB_WIRE_HD inline uint32_t modes_length(uint32_t df) { return df < 16u ? 7u : 14u; }

// S = crc24(b[0..len-3)) ^ b[len-3..len): 0 for an intact self-checking frame, the address for an address/parity one
ADSB_WIRE_HD inline uint32_t modes_syndrome(const ModesBytes &b)
{
    if (modes_length(b[0] >> 3) == 7u) return modes_crc24(b, 4) ^ (b[4] << 16 | b[5] << 8 | b[6]);
    return modes_crc24(b, 11) ^ (b[11] << 16 | b[12] << 8 | b[13]);
}

// Gray code of `bits` bits (<= 8) to binary
ADSB_WIRE_HD inline uint32_t modes_gray(uint32_t g)
{
    g ^= g >> 1;
    g ^= g >> 2;
    g ^= g >> 4;
    return g;
}

// The 13-bit AC field f (bit 12 .. 0 = C1 A1 C2 A2 C4 A4 M B1 Q B2 D2 B4 D4).  Returns the flags (ADSB_MODES_ALT,
// ADSB_MODES_ALT_METRIC or 0) and *feet.
ADSB_WIRE_HD inline uint32_t modes_altitude(uint32_t f, int32_t *feet)
{
    *feet = 0;
    if (f == 0) return 0;
    if (f & 0x40u) return ADSB_MODES_ALT_METRIC;
    if (f & 0x10u) { // Q = 1: 11 bits of 25 ft
        const uint32_t n = (f & 0x1F80u) >> 2 | (f & 0x20u) >> 1 | (f & 0xFu);
        *feet = 25 * (int32_t)n - 1000;
        return ADSB_MODES_ALT;
    }
    // Gillham: D2 D4 A1 A2 A4 B1 B2 B4 is a Gray code of 500 ft steps, C1 C2 C4 one of 100 ft steps that runs 1..5 and
    // back with every 500 ft step
    const uint32_t hg = (f >> 2 & 1u) << 7 | (f & 1u) << 6 | (f >> 11 & 1u) << 5 | (f >> 9 & 1u) << 4 | (f >> 7 & 1u) << 3 |
                        (f >> 5 & 1u) << 2 | (f >> 3 & 1u) << 1 | (f >> 1 & 1u);
    const uint32_t cg = (f >> 12 & 1u) << 2 | (f >> 10 & 1u) << 1 | (f >> 8 & 1u);
    const uint32_t h = modes_gray(hg);
    uint32_t c = modes_gray(cg) & 7u;
    if (c == 5u) c = 7u;
    else if (c == 7u) c = 5u;
    if (c == 0u || c > 5u) return 0;
    if (h & 1u) c = 6u - c;
    *feet = 500 * (int32_t)h + 100 * (int32_t)c - 1300;
    return ADSB_MODES_ALT;
}

// The 13-bit ID field as four octal digits read in decimal: 7700 reads 7700
ADSB_WIRE_HD inline uint32_t modes_squawk(uint32_t f)
{
    const uint32_t a = (f >> 7 & 1u) << 2 | (f >> 9 & 1u) << 1 | (f >> 11 & 1u);
    const uint32_t b = (f >> 1 & 1u) << 2 | (f >> 3 & 1u) << 1 | (f >> 5 & 1u);
    const uint32_t c = (f >> 8 & 1u) << 2 | (f >> 10 & 1u) << 1 | (f >> 12 & 1u);
    const uint32_t d = (f & 1u) << 2 | (f >> 2 & 1u) << 1 | (f >> 4 & 1u);
    return 1000u * a + 100u * b + 10u * c + d;
}

// character v (6 bits) of the ICAO set as kIcaoCharset of the field decode spells it ('_' is the space, '#' is none);
// *ok: a letter, a digit or the space
ADSB_WIRE_HD inline char modes_char(uint32_t v, bool *ok)
{
    *ok = true;
    if (v - 1u < 26u) return (char)('A' + v - 1u);
    if (v - 48u < 10u) return (char)('0' + v - 48u);
    if (v == 32u) return '_';
    *ok = false;
    return '#';
}

// The record of one frame before the known set is asked: SELF, PARITY and UNSUPPORTED are final; UNKNOWN becomes KNOWN
// when modes_is_known says so.  Every byte of the record is written.
ADSB_WIRE_HD inline adsb_modes_rec modes_first(const uint8_t *bytes)
{
    const ModesBytes b = modes_bytes(bytes);
    adsb_modes_rec r{};
    const uint32_t df = b[0] >> 3;
    r.df = (uint8_t)df;
    const bool ap = df == 0 || df == 4 || df == 5 || df == 16 || df == 20 || df == 21 || df >= 24;
    const bool squitter = df == 17 || df == 18;
    if (!ap && !squitter && df != 11) {
        r.kind = ADSB_MODES_UNSUPPORTED;
        return r;
    }
    const uint32_t s = modes_syndrome(b);
    const uint32_t aa = b[1] << 16 | b[2] << 8 | b[3];
    if (ap) {
        r.kind = ADSB_MODES_UNKNOWN;
        r.address = s;
    } else if (s == 0) {
        r.kind = ADSB_MODES_SELF;
        r.address = aa;
    } else if (df == 11 && (s & 0xFFFF80u) == 0) {
        r.kind = ADSB_MODES_UNKNOWN;
        r.address = aa;
        r.iid = (uint8_t)(s & 0x7Fu);
    } else {
        r.kind = ADSB_MODES_PARITY;
    }
    uint32_t flags = 0;
    if (!ap) r.ca = (uint8_t)(b[0] & 7u);
    const uint32_t f = (b[2] & 0x1Fu) << 8 | b[3];
    if (df == 4 || df == 5 || df == 20 || df == 21) {
        const uint32_t fs = b[0] & 7u;
        r.fs = (uint8_t)fs;
        r.dr = (uint8_t)(b[1] >> 3);
        r.um = (uint8_t)((b[1] & 7u) << 3 | b[2] >> 5);
        if (fs == 1 || fs == 3) flags |= ADSB_MODES_GROUND;
        if (fs >= 2 && fs <= 4) flags |= ADSB_MODES_ALERT;
        if (fs == 4 || fs == 5) flags |= ADSB_MODES_SPI;
    }
    if (df == 0 || df == 16) {
        if (b[0] >> 2 & 1u) flags |= ADSB_MODES_GROUND;
        r.ri = (uint8_t)((b[1] & 7u) << 1 | b[2] >> 7);
    }
    if (df == 0 || df == 4 || df == 16 || df == 20) {
        int32_t feet;
        flags |= modes_altitude(f, &feet);
        r.altitude_ft = feet;
    }
    if (df == 5 || df == 21) {
        r.squawk = (uint16_t)modes_squawk(f);
        flags |= ADSB_MODES_SQUAWK;
    }
    if ((df == 20 || df == 21) && b[4] == 0x20u) {
        const uint64_t bits = (b.w0 << 40 | b.w1 >> 24) >> 16; // bytes 5..10: 48 bits
        bool all = true;
        uint64_t text = 0; // the eight characters, the first in the low byte
        for (uint32_t k = 0; k < 8; ++k) {
            bool ok;
            text |= (uint64_t)(uint8_t)modes_char((uint32_t)(bits >> (42u - 6u * k)) & 0x3Fu, &ok) << (8u * k);
            all = all && ok;
        }
        r.callsign[0] = (char)text, r.callsign[1] = (char)(text >> 8), r.callsign[2] = (char)(text >> 16);
        r.callsign[3] = (char)(text >> 24), r.callsign[4] = (char)(text >> 32), r.callsign[5] = (char)(text >> 40);
        r.callsign[6] = (char)(text >> 48), r.callsign[7] = (char)(text >> 56);
        if (all) flags |= ADSB_MODES_CALLSIGN;
    }
    r.flags = (uint16_t)flags;
    return r;
}

// does this record teach its address to the frames behind it
ADSB_WIRE_HD inline bool modes_teaches(const adsb_modes_rec &r) { return r.kind == ADSB_MODES_SELF; }
// is its frame one the trackers may key on bytes[1..3]
ADSB_WIRE_HD inline bool modes_is_squitter(const adsb_modes_rec &r)
{
    return r.kind == ADSB_MODES_SELF && (r.df == 17 || r.df == 18);
}

// known[0 .. n_known) ascending and unique, first[k] = 0 for an address of known_in, else 1 + the list index of the
// first SELF frame with it.  Address a is known at list index j iff it is in known[] with first <= j.
ADSB_WIRE_HD inline bool modes_is_known(const uint32_t *known, const uint32_t *first, uint32_t n_known, uint32_t a, uint32_t j)
{
    uint32_t lo = 0, hi = n_known;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (known[mid] < a) lo = mid + 1u;
        else hi = mid;
    }
    return lo < n_known && known[lo] == a && first[lo] <= j;
}

// The argument rules both entry points share (host code).  known_host: known_in can be read here, and is checked.
inline int modes_args_check(const adsb_frame *frames, size_t n, const uint64_t *counts, uint32_t n_receivers,
                            const uint32_t *known_in, size_t n_known_in, bool known_host)
{
    if ((!frames && n) || (!known_in && n_known_in) || (uint64_t)n_known_in > (1ull << kModesAddressBits)) return ADSB_E_ARG;
    if ((uint64_t)n + (uint64_t)n_known_in > 0xFFFFFFFFull) return ADSB_E_CAPACITY;
    if (counts) {
        if (n_receivers < 1 || n_receivers > kModesMaxReceivers) return ADSB_E_ARG;
        uint64_t sum = 0;
        for (uint32_t r = 0; r < n_receivers; ++r) {
            if (counts[r] > (uint64_t)n - sum) return ADSB_E_ARG;
            sum += counts[r];
        }
        if (sum != (uint64_t)n) return ADSB_E_ARG;
    }
    if (known_host)
        for (size_t k = 0; k < n_known_in; ++k)
            if (known_in[k] >= kModesNoAddress || (k && known_in[k] <= known_in[k - 1])) return ADSB_E_ARG;
    return ADSB_OK;
}

} // namespace adsbk

#endif
