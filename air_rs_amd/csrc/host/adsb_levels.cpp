// adsb_levels.cpp -- CPU mirror of the device's per-frame power statistics (adsb_levels.hip): adsb_host_frame_levels and
// adsb_level_dbfs of include/adsb_host.h.  Plain C++, no device: the definition in adsb_hip.h restated sample by sample.
#include "../../../include/adsb_host.h"
#include "../adsb_levels.h"

#include <cmath>
#include <cstring>

namespace {

constexpr size_t kWindow = 240; // 16 preamble + 112 x 2 samples (reference src/adsb.rs:98)

template <typename T>
inline uint32_t power(const T *iq, size_t k)
{
    const int64_t i = iq[2 * k], q = iq[2 * k + 1];
    return (uint32_t)(i * i + q * q); // i16: at most 2^31, which uint32_t holds and int32_t does not
}

template <typename T>
void frame_level(const T *iq, size_t w, const uint8_t bytes[14], adsb_frame_level *out)
{
    uint64_t signal = 0, noise = 0;
    uint32_t pulse_max = 0, pulse_min = 0xFFFFFFFFu, quiet_max = 0, weak = 0;
    auto pulse = [&](uint32_t p) {
        signal += p;
        if (p > pulse_max) pulse_max = p;
        if (p < pulse_min) pulse_min = p;
    };
    auto quiet = [&](uint32_t p) {
        noise += p;
        if (p > quiet_max) quiet_max = p;
    };
    for (size_t k = 0; k < 16; ++k) { // demod.rs:20-24: the preamble's pulses
        const uint32_t p = power(iq, w + k);
        if (k == 0 || k == 2 || k == 7 || k == 9) pulse(p);
        else quiet(p);
    }
    for (size_t b = 0; b < 112; ++b) {
        const bool one = (bytes[b >> 3] >> (7 - (b & 7))) & 1;
        const uint32_t first = power(iq, w + 16 + 2 * b), second = power(iq, w + 16 + 2 * b + 1);
        const uint32_t hi = one ? first : second, lo = one ? second : first;
        pulse(hi);
        quiet(lo);
        if ((uint64_t)hi < 2 * (uint64_t)lo) ++weak;
    }
    out->signal_sum = signal;
    out->noise_sum = noise;
    out->peak = pulse_max > quiet_max ? pulse_max : quiet_max;
    out->pulse_min = pulse_min;
    out->quiet_max = quiet_max;
    out->weak_bits = (uint16_t)weak;
    out->flags = ADSB_LEVEL_VALID;
}

template <typename T>
void frame_levels(const T *iq, size_t n_samples, uint64_t first, const adsb_frame *frames, size_t n, adsb_frame_level *out)
{
    for (size_t i = 0; i < n; ++i) {
        std::memset(&out[i], 0, sizeof(out[i]));
        const uint64_t off = frames[i].offset;
        if (n_samples < kWindow || off < first || off - first > (uint64_t)(n_samples - kWindow)) continue;
        frame_level(iq, (size_t)(off - first), frames[i].bytes, &out[i]);
    }
}

} // namespace

extern "C" int adsb_host_frame_levels(int sample_type, const void *iq, size_t n_samples, uint64_t first_sample_index,
                                      const adsb_frame *frames, size_t n, adsb_frame_level *out)
{
    if (!iq || ((!frames || !out) && n)) return ADSB_E_ARG;
    if (sample_type == ADSB_SAMPLE_I8)
        frame_levels(static_cast<const int8_t *>(iq), n_samples, first_sample_index, frames, n, out);
    else if (sample_type == ADSB_SAMPLE_I16)
        frame_levels(static_cast<const int16_t *>(iq), n_samples, first_sample_index, frames, n, out);
    else
        return ADSB_E_ARG;
    return ADSB_OK;
}

namespace {

// adsb_levels_modes_of's records: ../adsb_levels.h's parts, which the device folds across a wave, taken in sequence
template <typename T>
void frame_levels_modes(const T *iq, uint32_t n_channels, size_t n_samples, size_t stride, uint64_t first,
                        const adsb_frame *frames, const uint64_t *counts, adsb_frame_level *out)
{
    using namespace adsbk;
    size_t i = 0;
    for (uint32_t c = 0; c < n_channels; ++c) {
        const T *chan = iq + 2 * stride * (size_t)c;
        for (uint64_t k = 0; k < counts[c]; ++k, ++i) {
            const adsb_frame &f = frames[i];
            const bool is_short = levels_is_short(f.bytes[0]);
            const bool valid = levels_inside(f.offset, first, n_samples, levels_window(is_short));
            LevelsPart t = levels_nothing();
            for (uint32_t l = 0; valid && l < levels_lanes(is_short); ++l) {
                uint32_t p[4];
                for (uint32_t s = 0; s < 4; ++s) p[s] = power(chan, (size_t)(f.offset - first) + kLevelsLaneSamples * l + s);
                t = levels_combine(t, levels_lane_part(l, p, l < 4u ? 0u : (uint32_t)f.bytes[(l - 4u) >> 2]));
            }
            out[i] = levels_record(t, valid, is_short);
        }
    }
}

} // namespace

extern "C" int adsb_host_frame_levels_modes(int sample_type, const void *iq, uint32_t n_channels, size_t n_samples,
                                            size_t channel_stride, uint64_t first_sample_index, const adsb_frame *frames,
                                            const uint64_t *counts, size_t n, adsb_frame_level *out)
{
    if ((sample_type != ADSB_SAMPLE_I8 && sample_type != ADSB_SAMPLE_I16) || (!out && n)) return ADSB_E_ARG;
    const int rc = adsbk::levels_modes_args_check(iq, n_channels, n_samples, channel_stride, frames, counts, n);
    if (rc != ADSB_OK) return rc;
    if (n_channels == 1) channel_stride = n_samples;
    if (sample_type == ADSB_SAMPLE_I8)
        frame_levels_modes(static_cast<const int8_t *>(iq), n_channels, n_samples, channel_stride, first_sample_index, frames, counts, out);
    else
        frame_levels_modes(static_cast<const int16_t *>(iq), n_channels, n_samples, channel_stride, first_sample_index, frames, counts, out);
    return ADSB_OK;
}

extern "C" double adsb_level_dbfs(int sample_type, uint64_t sum, uint32_t n_samples)
{
    if ((sample_type != ADSB_SAMPLE_I8 && sample_type != ADSB_SAMPLE_I16) || n_samples == 0) return NAN;
    if (sum == 0) return -INFINITY;
    const double full_scale = sample_type == ADSB_SAMPLE_I8 ? 32768.0 : 2147483648.0;
    return 10.0 * std::log10((double)sum / (double)n_samples / full_scale);
}
