// adsb_commb.hip -- the Comm-B register of every DF20/21 frame of a list and its values (adsb_commb_of,
// include/adsb_hip.h "Comm-B registers"; adsb_commb.h has the record of one frame, shared with the CPU mirror).
//
// Two steps in stream order, n known to the host and nothing read back in between:
//   1 commb_frames   one thread per frame j writes its record; a workgroup takes kT = 256 consecutive frames.  The
//                    stage is one read of 24 bytes and one write of 32 bytes per frame and a few dozen integer
//                    instructions between them, so how the bytes travel is what it costs.  A thread that loads its own
//                    frame reads 24-byte-strided addresses: every load instruction of a wave touches 12 cache lines
//                    for 8 bytes of each lane, and a record written by its thread is two 16-byte stores at a 32-byte
//                    stride.  Here the workgroup moves its 6144 bytes of frames as 768 consecutive 8-byte words, lane
//                    i at word i (frames are 8-byte aligned, not more: a caller's list may start at any frame), into
//                    LDS; each thread then reads bytes 0..15 of its frame as two 8-byte words (one ds_read2_b64; at a
//                    24-byte stride the 32 lanes of a half-wave start on 32 different even banks) and byte-swaps them
//                    into ModesBytes' big-endian words.  A full workgroup issues its three loads together.  The records go the same way back: packed into two uint4 per thread in LDS,
//                    then written as 512 consecutive uint4, lane i at uint4 i.  The workgroup's twelve counts (the five
//                    states and the ONE records of each register: wave ballots, then LDS) go to tally[].
//   2 commb_totals   ONE workgroup: the header from tally[], every byte of it.  A thread adds up every 256th
//                    workgroup's counts, eight workgroups per round with all 24 loads in flight at once: one thread
//                    per round would wait a memory latency for each (50 us at 8 Mi frames, measured, beside 116 us
//                    for step 1).
// No atomics, no workgroup waits for another (the dispatch boundary is the only ordering), plain stores, and nothing
// depends on the grid: the same bytes from run to run.  Everything a thread addresses: the frames' words [g] with
// g < 3 n; the records' uint4 [i] with i < 2 n; tally[12 b + k] with b < commb_blocks(n), k < 12; the header.
#include <hip/hip_runtime.h>

#include "adsb_commb.h"
#include "adsb_kernels.h"

namespace adsbk {

namespace {

constexpr uint32_t kT = kCommbBlock;
constexpr uint32_t kWaves = kT / 64;
constexpr uint32_t kK = kCommbTallyWords;
static_assert(kT % 64 == 0 && kK == kCommbTallies && kT >= kK, "whole waves, a thread per count");
static_assert(sizeof(adsb_frame) == 24 && sizeof(adsb_commb_rec) == 32, "three words in, two uint4 out");

// bytes 0..7 and 8..15 of a frame's bytes[] as the device loads them (little-endian words) -> ModesBytes
__device__ __forceinline__ ModesBytes commb_bytes(uint64_t lo, uint64_t hi)
{
    return ModesBytes{__builtin_bswap64(lo), __builtin_bswap64(hi) & ~0xFFFFull}; // (status and fixed_bit are no frame bytes)
}

__global__ __launch_bounds__(kT) void commb_frames(const CommbArgs a)
{
    __shared__ uint64_t in[3 * kT];
    __shared__ uint4 out[2 * kT];
    __shared__ uint32_t part[kWaves][kK];
    const uint32_t t = threadIdx.x;
    const uint64_t first = (uint64_t)blockIdx.x * kT;                     // the workgroup's first frame
    const uint32_t mine = (uint32_t)((uint64_t)a.n - first < kT ? (uint64_t)a.n - first : kT); // frames of it: 1..kT
    const uint64_t *src = reinterpret_cast<const uint64_t *>(a.frames) + 3u * first;
    if (mine == kT) { // (uniform) a whole workgroup's worth: the three loads are in flight together
        const uint64_t w0 = src[t], w1 = src[t + kT], w2 = src[t + 2u * kT];
        in[t] = w0, in[t + kT] = w1, in[t + 2u * kT] = w2;
    } else {
#pragma unroll
        for (uint32_t k = 0; k < 3; ++k) {
            const uint32_t w = t + k * kT;
            if (w < 3u * mine) in[w] = src[w];
        }
    }
    __syncthreads();
    uint32_t state = 0xFFu, reg = 0xFFu; // no frame
    if (t < mine) {
        const adsb_commb_rec r = commb_first(commb_bytes(in[3u * t + 1u], in[3u * t + 2u]));
        state = r.state;
        reg = commb_register_tally(r);
        out[2u * t] = make_uint4((uint32_t)r.state | (uint32_t)r.bds << 8 | (uint32_t)r.candidates << 16 | (uint32_t)r.n_candidates << 24,
                                 (uint32_t)r.status | (uint32_t)r.reserved << 16, (uint32_t)r.value[0], (uint32_t)r.value[1]);
        out[2u * t + 1u] = make_uint4((uint32_t)r.value[2], (uint32_t)r.value[3], (uint32_t)r.value[4], r.word);
    }
    const uint32_t lane = t & 63u, wave = t >> 6;
#pragma unroll
    for (uint32_t k = 0; k < kK; ++k) {
        const uint32_t c = (uint32_t)__popcll(__ballot(k < 5u ? state == k : reg == k));
        if (lane == 0) part[wave][k] = c;
    }
    __syncthreads();
    uint4 *dst = reinterpret_cast<uint4 *>(a.recs) + 2u * first;
#pragma unroll
    for (uint32_t k = 0; k < 2; ++k) {
        const uint32_t i = t + k * kT;
        if (i < 2u * mine) dst[i] = out[i];
    }
    if (t < kK) {
        uint32_t s = 0;
#pragma unroll
        for (uint32_t w = 0; w < kWaves; ++w) s += part[w][t];
        a.tally[kK * blockIdx.x + t] = s;
    }
}

__global__ __launch_bounds__(kT) void commb_totals(const CommbArgs a)
{
    __shared__ uint64_t part[kWaves][kK];
    const uint32_t blocks = commb_blocks(a.n);
    // a thread's share is at most blocks / kT workgroups' counts of at most kT each: below 2^32 / kT, 32 bits hold it.
    // Eight workgroups' twelve words per round, all loads issued before the first is waited for: the one workgroup
    // pays a memory latency per round, not per word
    uint32_t s[kK];
#pragma unroll
    for (uint32_t k = 0; k < kK; ++k) s[k] = 0;
    for (uint32_t b = threadIdx.x; b < blocks; b += 8u * kT) { // (blocks <= 2^24: b does not wrap)
        uint32_t w[8][kK];
#pragma unroll
        for (uint32_t i = 0; i < 8; ++i) {
            const uint32_t at = b + i * kT < blocks ? b + i * kT : blocks - 1u; // past the end: the last one again, not counted
#pragma unroll
            for (uint32_t k = 0; k < kK; ++k) w[i][k] = a.tally[kK * (size_t)at + k];
        }
#pragma unroll
        for (uint32_t i = 0; i < 8; ++i)
#pragma unroll
            for (uint32_t k = 0; k < kK; ++k) s[k] += b + i * kT < blocks ? w[i][k] : 0u;
    }
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
    for (uint32_t k = 0; k < kK; ++k) {
        uint64_t t = s[k];
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) t += __shfl_down(t, d, 64);
        if (lane == 0) part[wave][k] = t;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t total[kK];
#pragma unroll
        for (uint32_t k = 0; k < kK; ++k) {
            total[k] = 0;
#pragma unroll
            for (uint32_t w = 0; w < kWaves; ++w) total[k] += part[w][k];
        }
        commb_header_of(a.n, total, a.hdr);
    }
}

} // namespace

hipError_t launch_commb(hipStream_t st, const CommbArgs &a)
{
    if (a.n) hipLaunchKernelGGL(commb_frames, dim3(commb_blocks(a.n)), dim3(kT), 0, st, a);
    hipLaunchKernelGGL(commb_totals, dim3(1), dim3(kT), 0, st, a);
    return hipGetLastError();
}

} // namespace adsbk
