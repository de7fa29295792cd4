// adsb_es.hip -- the extended squitter status of every DF17/18 frame of a list (adsb_es_of, include/adsb_hip.h "Extended
// squitter status"; adsb_es.h has the record of one frame, shared with the CPU mirror).
//
// The shape of adsb_commb.hip, which moves the same 24 bytes in and 32 bytes out per frame.  Two steps in stream order,
// n known to the host and nothing read back in between:
//   1 es_frames   one thread per frame j writes its record; a workgroup takes kT = 256 consecutive frames.  How the
//                 bytes travel is what the stage costs: the workgroup moves its 6144 bytes of frames as 768 consecutive
//                 8-byte words, lane i at word i (frames are 8-byte aligned, not more: a caller's list may start at any
//                 frame), into LDS; each thread then reads bytes 0..15 of its frame as two 8-byte words (at a 24-byte
//                 stride the 32 lanes of a half-wave start on 32 different even banks) and byte-swaps them into
//                 ModesBytes' big-endian words.  A full workgroup issues its three loads together.  The records go the
//                 same way back: packed into two uint4 per thread in LDS, then written as 512 consecutive uint4, lane i
//                 at uint4 i.  The workgroup's fourteen counts (the ten states and the OPERATIONAL records of each
//                 version: wave ballots, then LDS) go to tally[].
//   2 es_totals   ONE workgroup: the header from tally[], every byte of it.  A thread adds up every 256th workgroup's
//                 counts, eight workgroups per round with all loads in flight at once.
// No atomics, no workgroup waits for another (the dispatch boundary is the only ordering), plain stores, and nothing
// depends on the grid: the same bytes from run to run.  Everything a thread addresses: the frames' words [g] with
// g < 3 n; the records' uint4 [i] with i < 2 n; tally[14 b + k] with b < es_blocks(n), k < 14; the header.
#include <hip/hip_runtime.h>

#include "adsb_es.h"
#include "adsb_kernels.h"

namespace adsbk {

namespace {

constexpr uint32_t kT = kEsBlock;
constexpr uint32_t kWaves = kT / 64;
constexpr uint32_t kK = kEsTallyWords;
static_assert(kT % 64 == 0 && kK == kEsTallies && kT >= kK, "whole waves, a thread per count");
static_assert(sizeof(adsb_frame) == 24 && sizeof(adsb_es_rec) == 32, "three words in, two uint4 out");

// bytes 0..7 and 8..15 of a frame's bytes[] as the device loads them (little-endian words) -> ModesBytes
__device__ __forceinline__ ModesBytes es_bytes(uint64_t lo, uint64_t hi)
{
    return ModesBytes{__builtin_bswap64(lo), __builtin_bswap64(hi) & ~0xFFFFull}; // (status and fixed_bit are no frame bytes)
}

__global__ __launch_bounds__(kT) void es_frames(const EsArgs a)
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
    uint32_t state = 0xFFu, ver = 0xFFu; // no frame
    if (t < mine) {
        const adsb_es_rec r = es_first(es_bytes(in[3u * t + 1u], in[3u * t + 2u]));
        state = r.state;
        ver = es_version_tally(r);
        out[2u * t] = make_uint4((uint32_t)r.state | (uint32_t)r.type_code << 8 | (uint32_t)r.subtype << 16 | (uint32_t)r.version << 24, r.present,
                                 (uint32_t)r.nic_a | (uint32_t)r.nic_b << 8 | (uint32_t)r.nic_c << 16 | (uint32_t)r.nac_p << 24,
                                 (uint32_t)r.nac_v | (uint32_t)r.sil << 8 | (uint32_t)r.sil_supplement << 16 | (uint32_t)r.gva << 24);
        out[2u * t + 1u] = make_uint4((uint32_t)r.sda | (uint32_t)r.nic_baro << 8 | (uint32_t)r.category << 16 | (uint32_t)r.emergency << 24,
                                      (uint32_t)r.length_width | (uint32_t)r.reserved << 8 | (uint32_t)r.flags << 16, r.value,
                                      (uint32_t)r.half[0] | (uint32_t)r.half[1] << 16);
    }
    const uint32_t lane = t & 63u, wave = t >> 6;
#pragma unroll
    for (uint32_t k = 0; k < kK; ++k) {
        const uint32_t c = (uint32_t)__popcll(__ballot(k < ADSB_ES_STATES ? state == k : ver == k));
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

__global__ __launch_bounds__(kT) void es_totals(const EsArgs a)
{
    __shared__ uint64_t part[kWaves][kK];
    const uint32_t blocks = es_blocks(a.n);
    // a thread's share is at most blocks / kT workgroups' counts of at most kT each: below 2^32 / kT, 32 bits hold it.
    // Eight workgroups' fourteen words per round, all loads issued before the first is waited for: the one workgroup
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
        es_header_of(a.n, total, a.hdr);
    }
}

} // namespace

hipError_t launch_es(hipStream_t st, const EsArgs &a)
{
    if (a.n) hipLaunchKernelGGL(es_frames, dim3(es_blocks(a.n)), dim3(kT), 0, st, a);
    hipLaunchKernelGGL(es_totals, dim3(1), dim3(kT), 0, st, a);
    return hipGetLastError();
}

} // namespace adsbk
