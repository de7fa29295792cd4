// adsb_levels.hip -- per-frame signal and noise power (adsb_levels_device_async / adsb_levels_of, include/adsb_hip.h):
// exact integer statistics of the 240 samples a frame was decoded from.  The reference's gate declares "signal power,
// noise power" (src/adsb/demod.rs:16-17) and returns zeros (demod.rs:56).
//
// One wavefront per frame, frames in a grid-stride loop.  Lane l < 60 owns the four window samples 4l .. 4l+3:
//   lanes 0-3   the preamble (pulses at 0, 2, 7, 9: demod.rs:20-24), a fixed pulse mask per lane;
//   lanes 4-59  the PPM pairs of bits 2l-8 and 2l-7, both in byte (l-4)/4 of the frame: one byte load per lane.
// Lanes 60-63 carry the reductions' identities.  Every load is naturally aligned and lies inside the lane's own four
// samples: i16 samples are dwords; an i8 window starts on a 2-byte boundary, so a lane's 8 bytes are two dwords when that
// address is dword-aligned and halfword + dword + halfword when it is not (wave-uniform: lanes are 8 bytes apart).
// Nothing is rounded up or down to an alignment, so nothing outside [w, w + 240) of the frame's channel is addressed.
// The two sums, two maxima, the minimum and the weak-bit count are reduced across the wave in registers; lane 0 stores
// the 32-byte record.  No LDS, no scratch, no atomics: a latency-bound epilogue of 480 / 960 + 56 bytes per frame.
// frame_levels_modes_kernel below (adsb_levels_modes_of) is the same plan for a list of 56-bit and 112-bit frames.
#include "adsb_kernels.h"
#include "adsb_levels.h"
#include "adsb_replies.h"

namespace adsbk {

namespace {

__device__ __forceinline__ uint32_t uniform(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ uint64_t uniform64(uint64_t v)
{
    return ((uint64_t)uniform((uint32_t)(v >> 32)) << 32) | uniform((uint32_t)v);
}

template <typename T>
__device__ __forceinline__ T wave_sum(T v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}
__device__ __forceinline__ uint32_t wave_max(uint32_t v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) { const uint32_t o = __shfl_xor(v, m, 64); v = o > v ? o : v; }
    return v;
}
__device__ __forceinline__ uint32_t wave_min(uint32_t v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) { const uint32_t o = __shfl_xor(v, m, 64); v = o < v ? o : v; }
    return v;
}

// p = I^2 + Q^2 of the lane's four samples at `at` (the lane's first sample; aligned to one sample)
template <int ST>
__device__ __forceinline__ void lane_powers(const char *at, bool dword_aligned, uint32_t p[4])
{
    if (ST == ADSB_SAMPLE_I16) {
        const uint32_t *d = reinterpret_cast<const uint32_t *>(at);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t s = d[k];
            const int32_t i = (int16_t)(s & 0xFFFFu), q = (int16_t)(s >> 16);
            p[k] = (uint32_t)(i * i) + (uint32_t)(q * q); // up to 2^31: unsigned
        }
    } else {
        uint32_t s[4];
        if (dword_aligned) {
            const uint32_t d0 = *reinterpret_cast<const uint32_t *>(at), d1 = *reinterpret_cast<const uint32_t *>(at + 4);
            s[0] = d0 & 0xFFFFu; s[1] = d0 >> 16; s[2] = d1 & 0xFFFFu; s[3] = d1 >> 16;
        } else {
            const uint32_t h0 = *reinterpret_cast<const uint16_t *>(at);
            const uint32_t d = *reinterpret_cast<const uint32_t *>(at + 2);
            const uint32_t h1 = *reinterpret_cast<const uint16_t *>(at + 6);
            s[0] = h0; s[1] = d & 0xFFFFu; s[2] = d >> 16; s[3] = h1;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int32_t i = (int8_t)(s[k] & 0xFFu), q = (int8_t)(s[k] >> 8);
            p[k] = (uint32_t)(i * i + q * q);
        }
    }
}

template <int ST>
__global__ __launch_bounds__(256) void frame_levels_kernel(const LevelsArgs a)
{
    constexpr uint32_t kBps = ST == ADSB_SAMPLE_I8 ? 2u : 4u;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t waves_per_block = blockDim.x >> 6;
    const uint32_t n_waves = gridDim.x * waves_per_block;
    const uint64_t n64 = a.hdr ? a.hdr->n_out : (uint64_t)a.cap;
    const uint32_t n = uniform(n64 < a.cap ? (uint32_t)n64 : a.cap);
    // (a 64-bit counter: i + n_waves must not wrap for a list of nearly 2^32 frames)
    for (uint64_t i = uniform(blockIdx.x * waves_per_block + (threadIdx.x >> 6)); i < n; i += n_waves) {
        const adsb_frame *f = a.frames + i;
        const uint64_t off = uniform64(f->offset);
        // the frame's window inside its channel: [w, w + 240) must lie in [0, n_samples)
        const bool valid = a.n_samples >= (uint64_t)kWindow && off >= a.offset_base &&
                           off - a.offset_base <= a.n_samples - (uint64_t)kWindow;
        uint64_t signal = 0, noise = 0;
        uint32_t pulse_max = 0, pulse_min = 0xFFFFFFFFu, quiet_max = 0, weak = 0;
        if (valid) {
            // channel of frame i: how many of the channels 1 .. n_channels-1 start at or before it in the list
            uint32_t chan = 0;
            for (uint32_t c0 = 1; c0 < a.n_channels; c0 += 64) {
                const uint32_t c = c0 + lane;
                const bool before = c < a.n_channels && a.chan_prefix[c] <= i;
                chan += (uint32_t)__popcll(__ballot(before));
            }
            chan = uniform(chan);
            const uint64_t first = (uint64_t)chan * a.channel_stride + (off - a.offset_base); // sample index of w
            const char *win = static_cast<const char *>(a.iq) + first * kBps;
            const bool dword_aligned = (uniform((uint32_t)(uintptr_t)win) & 2u) == 0;
            if (lane < 60) {
                uint32_t p[4];
                lane_powers<ST>(win + lane * 4u * kBps, dword_aligned, p);
                uint32_t mask; // bit k: the lane's sample k is a pulse sample
                if (lane < 4) {
                    mask = lane == 0 ? 0x5u : lane == 1 ? 0x8u : lane == 2 ? 0x2u : 0x0u; // window samples 0, 2 | 7 | 9
                } else {
                    const uint32_t byte = f->bytes[(lane - 4u) >> 2];
                    const uint32_t k = (lane - 4u) & 3u;                  // bits 2k and 2k+1 of that byte, MSB first
                    const uint32_t b0 = (byte >> (7u - 2u * k)) & 1u, b1 = (byte >> (6u - 2u * k)) & 1u;
                    mask = (b0 ? 0x1u : 0x2u) | (b1 ? 0x4u : 0x8u);
                    const uint32_t hi0 = b0 ? p[0] : p[1], lo0 = b0 ? p[1] : p[0];
                    const uint32_t hi1 = b1 ? p[2] : p[3], lo1 = b1 ? p[3] : p[2];
                    weak = ((uint64_t)hi0 < 2 * (uint64_t)lo0 ? 1u : 0u) + ((uint64_t)hi1 < 2 * (uint64_t)lo1 ? 1u : 0u);
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if ((mask >> k) & 1u) {
                        signal += p[k];
                        pulse_max = p[k] > pulse_max ? p[k] : pulse_max;
                        pulse_min = p[k] < pulse_min ? p[k] : pulse_min;
                    } else {
                        noise += p[k];
                        quiet_max = p[k] > quiet_max ? p[k] : quiet_max;
                    }
                }
            }
            signal = wave_sum(signal);
            noise = wave_sum(noise);
            weak = wave_sum(weak);
            pulse_max = wave_max(pulse_max);
            quiet_max = wave_max(quiet_max);
            pulse_min = wave_min(pulse_min);
        }
        if (lane == 0) {
            adsb_frame_level r;
            r.signal_sum = signal;
            r.noise_sum = noise;
            r.peak = pulse_max > quiet_max ? pulse_max : quiet_max;
            r.pulse_min = valid ? pulse_min : 0u;
            r.quiet_max = quiet_max;
            r.weak_bits = (uint16_t)weak;
            r.flags = valid ? (uint16_t)ADSB_LEVEL_VALID : (uint16_t)0;
            a.out[i] = r;
        }
    }
}

// Level records by frame length (adsb_levels_modes_of): the same shape over a caller's list of short and long frames
// from many channels.  A short frame's window is 128 samples: lanes 0-31 own them, lanes 4-31 read bytes 0..6, and
// lanes 32-63 address nothing and carry the identities, as lanes 60-63 do for a long frame.  The frame's channel is a
// binary search of the list's prefix (wave-uniform: every lane runs it on the same index).  The per-lane text, the
// window test and the record are adsb_levels.h's, which the CPU mirror compiles too.
template <int ST>
__global__ __launch_bounds__(256) void frame_levels_modes_kernel(const LevelsModesArgs a)
{
    constexpr uint32_t kBps = ST == ADSB_SAMPLE_I8 ? 2u : 4u;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t waves_per_block = blockDim.x >> 6;
    const uint32_t n_waves = gridDim.x * waves_per_block;
    for (uint64_t i = uniform(blockIdx.x * waves_per_block + (threadIdx.x >> 6)); i < a.n; i += n_waves) {
        const adsb_frame *f = a.frames + i;
        const uint64_t off = uniform64(f->offset);
        const bool is_short = levels_is_short(uniform(f->bytes[0]));
        const bool valid = levels_inside(off, a.offset_base, a.n_samples, levels_window(is_short));
        LevelsPart t = levels_nothing();
        if (valid) {
            const uint32_t chan = a.n_channels > 1 ? uniform(replies_channel_of(a.prefix, a.n_channels, i)) : 0u;
            const uint64_t first = (uint64_t)chan * a.channel_stride + (off - a.offset_base); // sample index of w
            const char *win = static_cast<const char *>(a.iq) + first * kBps;
            const bool dword_aligned = (uniform((uint32_t)(uintptr_t)win) & 2u) == 0;
            if (lane < levels_lanes(is_short)) {
                uint32_t p[4];
                lane_powers<ST>(win + lane * kLevelsLaneSamples * kBps, dword_aligned, p);
                t = levels_lane_part(lane, p, lane < 4u ? 0u : (uint32_t)f->bytes[(lane - 4u) >> 2]);
            }
            t.signal = wave_sum(t.signal);
            t.noise = wave_sum(t.noise);
            t.weak = wave_sum(t.weak);
            t.pulse_max = wave_max(t.pulse_max);
            t.quiet_max = wave_max(t.quiet_max);
            t.pulse_min = wave_min(t.pulse_min);
        }
        if (lane == 0) a.out[i] = levels_record(t, valid, is_short);
    }
}

} // namespace

hipError_t launch_frame_levels_modes(hipStream_t s, int sample_type, const LevelsModesArgs &a, uint32_t blocks)
{
    if (a.n == 0 || blocks == 0) return hipSuccess;
    if (sample_type == ADSB_SAMPLE_I8)
        hipLaunchKernelGGL(frame_levels_modes_kernel<ADSB_SAMPLE_I8>, dim3(blocks), dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL(frame_levels_modes_kernel<ADSB_SAMPLE_I16>, dim3(blocks), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_frame_levels(hipStream_t s, int sample_type, const LevelsArgs &a, uint32_t blocks)
{
    if (a.cap == 0 || blocks == 0) return hipSuccess;
    if (sample_type == ADSB_SAMPLE_I8)
        hipLaunchKernelGGL(frame_levels_kernel<ADSB_SAMPLE_I8>, dim3(blocks), dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL(frame_levels_kernel<ADSB_SAMPLE_I16>, dim3(blocks), dim3(256), 0, s, a);
    return hipGetLastError();
}

} // namespace adsbk
