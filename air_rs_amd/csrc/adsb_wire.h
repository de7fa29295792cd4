// adsb_wire.h -- one frame as Beast binary or AVR text (include/adsb_hip.h, "Wire output"): the signal byte, the 21
// payload bytes, the escaped length, the hex digits and the encoder itself.  One text for the device (adsb_wire.hip, one
// thread per frame) and the CPU mirror (host/adsb_wire.cpp, adsb_host_wire_encode): every function here is
// __host__ __device__ under hipcc and plain inline C++ otherwise.  Integers only, so both sides agree to the bit.
#ifndef ADSB_WIRE_H
#define ADSB_WIRE_H

#include <stdint.h>

#include "../../include/adsb_hip.h"

#if defined(__HIPCC__)
#define ADSB_WIRE_HD __host__ __device__
#else
#define ADSB_WIRE_HD
#endif

namespace adsbk {

constexpr uint32_t kWirePayload = 21;                 // 6 bytes of timestamp, the signal byte, 14 frame bytes
constexpr uint32_t kWireMaxBytes = ADSB_WIRE_MAX_BYTES; // 1A 33 + every payload byte doubled
constexpr uint32_t kWireAvrBytes = 31, kWireAvrMlatBytes = 43;
constexpr uint64_t kWireTickMask = (1ull << 48) - 1;

ADSB_WIRE_HD inline bool wire_cfg_ok(const adsb_wire_cfg *cfg)
{
    return cfg && cfg->format <= ADSB_WIRE_AVR_MLAT && cfg->tick_bias <= kWireTickMask;
}

// The 12 MHz timestamp of a frame: six ticks per 2 MSPS sample, 48 bits (2^48 divides 2^64: the product may wrap).
ADSB_WIRE_HD inline uint64_t wire_ticks(uint64_t offset, uint64_t tick_bias)
{
    return (6ull * offset + tick_bias) & kWireTickMask;
}

// 255 sqrt(signal_sum / (116 FS)) rounded half up, clamped to 255, at least 1 for a sum above zero: the largest s in
// 0..255 with (2s-1)^2 116 FS <= 4 255^2 signal_sum.  A sum above 116 FS (no window of samples adds up to one) counts as
// 116 FS, which gives 255 already, so that the right side stays below 2^64.
ADSB_WIRE_HD inline uint32_t wire_signal_byte(uint64_t signal_sum, int sample_type)
{
    if (signal_sum == 0) return 0;
    const uint64_t unit = 116ull * (sample_type == ADSB_SAMPLE_I8 ? 32768ull : 2147483648ull);
    const uint64_t rhs = 4ull * 255ull * 255ull * (signal_sum < unit ? signal_sum : unit);
    uint32_t s = 0;
    for (uint32_t bit = 128; bit; bit >>= 1) { // the condition is monotone in s >= 1
        const uint64_t c = 2ull * (s | bit) - 1ull;
        if (c * c * unit <= rhs) s |= bit;
    }
    return s ? s : 1u;
}

// the signal byte of a frame from its level record (null: none)
ADSB_WIRE_HD inline uint32_t wire_signal_of(const adsb_frame_level *lv, int sample_type)
{
    return lv && (lv->flags & ADSB_LEVEL_VALID) ? wire_signal_byte(lv->signal_sum, sample_type) : 0u;
}

// payload byte k (0..20): the timestamp big-endian, the signal byte, the frame
ADSB_WIRE_HD inline uint32_t wire_payload_byte(uint32_t k, uint64_t t, uint32_t s, const uint8_t *bytes)
{
    return k < 6 ? (uint32_t)(t >> (40u - 8u * k)) & 0xFFu : k == 6 ? s : bytes[k - 7];
}

ADSB_WIRE_HD inline uint32_t wire_length(uint32_t format, uint64_t t, uint32_t s, const uint8_t *bytes)
{
    if (format == ADSB_WIRE_AVR) return kWireAvrBytes;
    if (format == ADSB_WIRE_AVR_MLAT) return kWireAvrMlatBytes;
    uint32_t n = 2 + kWirePayload;
    for (uint32_t k = 0; k < kWirePayload; ++k) n += wire_payload_byte(k, t, s, bytes) == 0x1Au ? 1u : 0u;
    return n;
}

ADSB_WIRE_HD inline uint8_t wire_hex(uint32_t nibble) // upper case
{
    return (uint8_t)(nibble < 10 ? '0' + nibble : 'A' + (nibble - 10));
}

// Writes the frame at dst (wire_length bytes of it) and returns that length.
ADSB_WIRE_HD inline uint32_t wire_encode(uint32_t format, uint64_t t, uint32_t s, const uint8_t *bytes, uint8_t *dst)
{
    uint32_t n = 0;
    if (format == ADSB_WIRE_BEAST) {
        dst[n++] = 0x1A;
        dst[n++] = 0x33;
        for (uint32_t k = 0; k < kWirePayload; ++k) {
            const uint32_t b = wire_payload_byte(k, t, s, bytes);
            dst[n++] = (uint8_t)b;
            if (b == 0x1Au) dst[n++] = 0x1A;
        }
        return n;
    }
    if (format == ADSB_WIRE_AVR_MLAT) {
        dst[n++] = '@';
        for (uint32_t k = 0; k < 12; ++k) dst[n++] = wire_hex((uint32_t)(t >> (44u - 4u * k)) & 0xFu);
    } else {
        dst[n++] = '*';
    }
    for (uint32_t k = 0; k < 14; ++k) {
        dst[n++] = wire_hex(bytes[k] >> 4);
        dst[n++] = wire_hex(bytes[k] & 0xFu);
    }
    dst[n++] = ';';
    dst[n++] = '\n';
    return n;
}

} // namespace adsbk

#endif
