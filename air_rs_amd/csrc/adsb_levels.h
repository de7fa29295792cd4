// adsb_levels.h -- one frame's level record by frame length (include/adsb_hip.h, "Level records by frame length"): the
// frame's window, whether it lies inside its channel, what one lane's four samples add to the record, how two parts
// combine, and the record itself.  One text for the device (adsb_levels.hip, frame_levels_modes_kernel: one wavefront
// per frame, one lane per part) and the CPU mirror (host/adsb_levels.cpp, adsb_host_frame_levels_modes: the parts in
// sequence): every function here is __host__ __device__ under hipcc and plain inline C++ otherwise.  Integers only.
#ifndef ADSB_LEVELS_H
#define ADSB_LEVELS_H

#include <stdint.h>

#include "../../include/adsb_hip.h"
#include "adsb_modes.h"

namespace adsbk {

constexpr uint32_t kLevelsLongWindow = 240;  // 16 + 2 x 112 samples
constexpr uint32_t kLevelsShortWindow = 128; // 16 + 2 x 56
constexpr uint32_t kLevelsLaneSamples = 4;   // window samples 4l .. 4l+3 are lane l's

ADSB_WIRE_HD inline bool levels_is_short(uint32_t byte0) { return modes_length(byte0 >> 3) == 7u; }
ADSB_WIRE_HD inline uint32_t levels_window(bool is_short) { return is_short ? kLevelsShortWindow : kLevelsLongWindow; }
// lanes that own samples: 32 of a short frame, 60 of a long one
ADSB_WIRE_HD inline uint32_t levels_lanes(bool is_short) { return levels_window(is_short) / kLevelsLaneSamples; }
// [w, w + window) with w = offset - offset_base lies inside [0, n_samples)
ADSB_WIRE_HD inline bool levels_inside(uint64_t offset, uint64_t offset_base, uint64_t n_samples, uint32_t window)
{
    return n_samples >= window && offset >= offset_base && offset - offset_base <= n_samples - window;
}

// What a set of samples adds to a record; the identity is the empty set.
struct LevelsPart {
    uint64_t signal, noise;
    uint32_t pulse_max, pulse_min, quiet_max, weak;
};
ADSB_WIRE_HD inline LevelsPart levels_nothing() { return LevelsPart{0, 0, 0, 0xFFFFFFFFu, 0, 0}; }
ADSB_WIRE_HD inline LevelsPart levels_combine(const LevelsPart &a, const LevelsPart &b)
{
    return LevelsPart{a.signal + b.signal, a.noise + b.noise, a.pulse_max > b.pulse_max ? a.pulse_max : b.pulse_max,
                      a.pulse_min < b.pulse_min ? a.pulse_min : b.pulse_min,
                      a.quiet_max > b.quiet_max ? a.quiet_max : b.quiet_max, a.weak + b.weak};
}

// Lane l's part (l < levels_lanes) from the powers p[0..4) of window samples 4l .. 4l+3.  Lanes 0-3 hold the preamble
// (pulses at 0, 2, 7, 9); lane l >= 4 holds the PPM pairs of bits 2l-8 and 2l-7, both in frame byte (l-4)/4, which is
// `byte` (not read for l < 4).  A short frame's lanes end at 31, so its bytes end at 6.
ADSB_WIRE_HD inline LevelsPart levels_lane_part(uint32_t l, const uint32_t p[4], uint32_t byte)
{
    LevelsPart r = levels_nothing();
    uint32_t mask; // bit k: sample k of the four is a pulse sample
    if (l < 4u) {
        mask = l == 0u ? 0x5u : l == 1u ? 0x8u : l == 2u ? 0x2u : 0x0u;
    } else {
        const uint32_t k = (l - 4u) & 3u; // bits 2k and 2k+1 of the byte, MSB first
        const uint32_t b0 = (byte >> (7u - 2u * k)) & 1u, b1 = (byte >> (6u - 2u * k)) & 1u;
        mask = (b0 ? 0x1u : 0x2u) | (b1 ? 0x4u : 0x8u);
        const uint32_t hi0 = b0 ? p[0] : p[1], lo0 = b0 ? p[1] : p[0];
        const uint32_t hi1 = b1 ? p[2] : p[3], lo1 = b1 ? p[3] : p[2];
        r.weak = ((uint64_t)hi0 < 2u * (uint64_t)lo0 ? 1u : 0u) + ((uint64_t)hi1 < 2u * (uint64_t)lo1 ? 1u : 0u);
    }
    for (uint32_t k = 0; k < 4u; ++k) {
        if ((mask >> k) & 1u) {
            r.signal += p[k];
            r.pulse_max = p[k] > r.pulse_max ? p[k] : r.pulse_max;
            r.pulse_min = p[k] < r.pulse_min ? p[k] : r.pulse_min;
        } else {
            r.noise += p[k];
            r.quiet_max = p[k] > r.quiet_max ? p[k] : r.quiet_max;
        }
    }
    return r;
}

// the record of a frame from all its lanes' parts combined; a frame whose window is not inside its channel gets zeros
ADSB_WIRE_HD inline adsb_frame_level levels_record(const LevelsPart &t, bool valid, bool is_short)
{
    adsb_frame_level r;
    r.signal_sum = valid ? t.signal : 0u;
    r.noise_sum = valid ? t.noise : 0u;
    r.peak = valid ? (t.pulse_max > t.quiet_max ? t.pulse_max : t.quiet_max) : 0u;
    r.pulse_min = valid ? t.pulse_min : 0u;
    r.quiet_max = valid ? t.quiet_max : 0u;
    r.weak_bits = (uint16_t)(valid ? t.weak : 0u);
    r.flags = (uint16_t)(valid ? (is_short ? ADSB_LEVEL_VALID | ADSB_LEVEL_SHORT : ADSB_LEVEL_VALID) : 0u);
    return r;
}

// The argument rules the device and the host entry points share (host code): counts[] is host memory and adds up to n.
inline int levels_modes_args_check(const void *iq, uint32_t n_channels, size_t n_samples, size_t channel_stride,
                                   const adsb_frame *frames, const uint64_t *counts, size_t n)
{
    if (!iq || !counts || (!frames && n)) return ADSB_E_ARG;
    if (n_channels == 0 || n_channels > (1u << 20)) return ADSB_E_ARG;
    if (n_channels > 1 && channel_stride < n_samples) return ADSB_E_ARG;
    if (n > 0xFFFFFFFFull) return ADSB_E_CAPACITY;
    uint64_t total = 0;
    for (uint32_t c = 0; c < n_channels; ++c) {
        if (counts[c] > (uint64_t)n - total) return ADSB_E_ARG;
        total += counts[c];
    }
    return total == (uint64_t)n ? ADSB_OK : ADSB_E_ARG;
}

} // namespace adsbk

#endif
