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
    return cfg && (cfg->format & ~ADSB_WIRE_SHORT) <= ADSB_WIRE_AVR_MLAT && cfg->tick_bias <= kWireTickMask;
}
// the format without the ADSB_WIRE_SHORT bit
ADSB_WIRE_HD inline uint32_t wire_base_format(uint32_t format) { return format & ~ADSB_WIRE_SHORT; }
// Frame bytes that are written: 7 with ADSB_WIRE_SHORT for a frame whose DF is below 16 (modes_length's rule;
// adsb_modes.h includes this file), else 14.  Nothing past them is read.
ADSB_WIRE_HD inline uint32_t wire_frame_bytes(uint32_t format, const uint8_t *bytes)
{
    return (format & ADSB_WIRE_SHORT) && (bytes[0] >> 3) < 16u ? 7u : 14u;
}

// The 12 MHz timestamp of a frame: six ticks per 2 MSPS sample, 48 bits (2^48 divides 2^64: the product may wrap).
ADSB_WIRE_HD inline uint64_t wire_ticks(uint64_t offset, uint64_t tick_bias)
{
    return (6ull * offset + tick_bias) & kWireTickMask;
}

// 255 sqrt(signal_sum / (P FS)) rounded half up, clamped to 255, at least 1 for a sum above zero, P = `pulses` the
// pulse samples the sum is over (116; 60 of a short frame's record): the largest s in 0..255 with (2s-1)^2 P FS <=
// 4 255^2 signal_sum.  A sum above P FS (no window of samples adds up to one) counts as P FS, which gives 255 already,
// so that the right side stays below 2^64.
ADSB_WIRE_HD inline uint32_t wire_signal_byte(uint64_t signal_sum, int sample_type, uint32_t pulses = 116u)
{
    if (signal_sum == 0) return 0;
    const uint64_t unit = (uint64_t)pulses * (sample_type == ADSB_SAMPLE_I8 ? 32768ull : 2147483648ull);
    const uint64_t rhs = 4ull * 255ull * 255ull * (signal_sum < unit ? signal_sum : unit);
    uint32_t s = 0;
    for (uint32_t bit = 128; bit; bit >>= 1) { // the condition is monotone in s >= 1
        const uint64_t c = 2ull * (s | bit) - 1ull;
        if (c * c * unit <= rhs) s |= bit;
    }
    return s ? s : 1u;
}

// the signal byte of a frame from its level record (null: none).  With ADSB_WIRE_SHORT in the format a record with
// ADSB_LEVEL_SHORT is a sum over 60 pulse samples; without the bit every record counts as one over 116.
ADSB_WIRE_HD inline uint32_t wire_signal_of(const adsb_frame_level *lv, int sample_type, uint32_t format)
{
    if (!lv || !(lv->flags & ADSB_LEVEL_VALID)) return 0u;
    const bool sixty = (format & ADSB_WIRE_SHORT) && (lv->flags & ADSB_LEVEL_SHORT);
    return wire_signal_byte(lv->signal_sum, sample_type, sixty ? 60u : 116u);
}

// payload byte k (0..20; 0..13 of a short frame): the timestamp big-endian, the signal byte, the frame
ADSB_WIRE_HD inline uint32_t wire_payload_byte(uint32_t k, uint64_t t, uint32_t s, const uint8_t *bytes)
{
    return k < 6 ? (uint32_t)(t >> (40u - 8u * k)) & 0xFFu : k == 6 ? s : bytes[k - 7];
}

ADSB_WIRE_HD inline uint32_t wire_length(uint32_t format, uint64_t t, uint32_t s, const uint8_t *bytes)
{
    const uint32_t fb = wire_frame_bytes(format, bytes), payload = 7u + fb;
    if (wire_base_format(format) == ADSB_WIRE_AVR) return kWireAvrBytes - 2u * (14u - fb);
    if (wire_base_format(format) == ADSB_WIRE_AVR_MLAT) return kWireAvrMlatBytes - 2u * (14u - fb);
    uint32_t n = 2 + payload;
    for (uint32_t k = 0; k < payload; ++k) n += wire_payload_byte(k, t, s, bytes) == 0x1Au ? 1u : 0u;
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
    const uint32_t fb = wire_frame_bytes(format, bytes);
    if (wire_base_format(format) == ADSB_WIRE_BEAST) {
        dst[n++] = 0x1A;
        dst[n++] = fb == 7u ? 0x32 : 0x33;
        for (uint32_t k = 0; k < 7u + fb; ++k) {
            const uint32_t b = wire_payload_byte(k, t, s, bytes);
            dst[n++] = (uint8_t)b;
            if (b == 0x1Au) dst[n++] = 0x1A;
        }
        return n;
    }
    if (wire_base_format(format) == ADSB_WIRE_AVR_MLAT) {
        dst[n++] = '@';
        for (uint32_t k = 0; k < 12; ++k) dst[n++] = wire_hex((uint32_t)(t >> (44u - 4u * k)) & 0xFu);
    } else {
        dst[n++] = '*';
    }
    for (uint32_t k = 0; k < fb; ++k) {
        dst[n++] = wire_hex(bytes[k] >> 4);
        dst[n++] = wire_hex(bytes[k] & 0xFu);
    }
    dst[n++] = ';';
    dst[n++] = '\n';
    return n;
}

} // namespace adsbk

#endif
