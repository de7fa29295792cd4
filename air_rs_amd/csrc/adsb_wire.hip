// adsb_wire.hip -- an ordered frame list as ONE contiguous stream of Beast binary or AVR text (adsb_wire_device_async /
// adsb_wire_of, include/adsb_hip.h "Wire output"; adsb_wire.h has the encoder, shared with the CPU mirror).
//
// Beast frames are 23..44 bytes long (every 0x1A of the 21 payload bytes is doubled), so where a frame's bytes go
// depends on every frame before it.  Three dispatches, in stream order, the frame count read on the device:
//   1 wire_lengths  one thread per frame, kWireBlockFrames frames per workgroup: the frame's encoded length, an
//                   inclusive scan of the lengths across the workgroup (registers, then one LDS word per wave), the
//                   workgroup-local end of every frame into ends[] and the workgroup's total into block[].  Workgroups
//                   past the count write a total of zero.
//   2 wire_totals   ONE workgroup turns block[] into the exclusive prefix of the totals (where each workgroup's span
//                   starts), kWireScanThreads at a time with a running carry, and writes the stream's header.
//   3 wire_write    every workgroup encodes its frames into LDS at their local positions -- its span of the stream,
//                   contiguous because frames are in order -- and stores the span cooperatively: bytes up to the first
//                   dword-aligned address, dwords (64 lanes x 4 bytes, consecutive) for the body, bytes for the tail.
//                   The LDS image starts at (span start mod 4), so a body dword is one aligned LDS dword; the body lies
//                   wholly inside the span, so no store covers a byte of a neighbouring workgroup's span.  ends[] become
//                   global here.
// No atomics, no workgroup waits for another (the dispatch boundaries are the only ordering), and nothing depends on
// the grid: the stream is the same bytes from run to run.  The fixed-length AVR forms take the same path with constant
// lengths.  Everything a thread addresses: frames[i], levels[i], ends[i] for i < min(count, cap); block[b] for b < grid;
// out[g] for g < the stream's length <= 44 x cap (the reserve checks that this fits 32 bits).
#include "adsb_kernels.h"
#include "adsb_wire.h"

namespace adsbk {

namespace {

constexpr uint32_t kWaves = kWireBlockFrames / 64;
static_assert(kWireBlockFrames % 64 == 0 && kWireScanThreads % 64 == 0, "whole waves");
// the LDS image of a span: the largest span plus the up to 3 bytes in front that align it like the stream
constexpr uint32_t kStageWords = (kWireBlockFrames * kWireMaxBytes + 3) / 4 + 1;

__device__ __forceinline__ uint32_t list_count(const WireArgs &a)
{
    const uint64_t n64 = a.hdr ? a.hdr->n_out : (uint64_t)a.cap;
    return n64 < a.cap ? (uint32_t)n64 : a.cap;
}

// inclusive scan of v across a workgroup of W waves; part: W words of LDS.  Every thread of the workgroup calls it.
template <uint32_t W>
__device__ __forceinline__ uint32_t block_inclusive_scan(uint32_t v, uint32_t *part)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(v, d, 64);
        if (lane >= (uint32_t)d) v += o;
    }
    if (lane == 63) part[wave] = v;
    __syncthreads();
    uint32_t before = 0;
#pragma unroll
    for (uint32_t w = 0; w < W; ++w) before += w < wave ? part[w] : 0u;
    __syncthreads(); // part[] may be written again by the caller's next round
    return v + before;
}

__device__ __forceinline__ void frame_stamp(const WireArgs &a, uint32_t i, const adsb_frame &f, uint64_t *t, uint32_t *s)
{
    *t = wire_ticks(f.offset, a.tick_bias);
    *s = a.levels ? wire_signal_of(a.levels + i, a.sample_type, a.format) : 0u;
}

__global__ __launch_bounds__(kWireBlockFrames) void wire_lengths(const WireArgs a)
{
    __shared__ uint32_t part[kWaves];
    const uint32_t n = list_count(a);
    const uint32_t i = blockIdx.x * kWireBlockFrames + threadIdx.x;
    uint32_t len = 0;
    if (i < n) {
        const adsb_frame f = a.frames[i];
        uint64_t t;
        uint32_t s;
        frame_stamp(a, i, f, &t, &s);
        len = wire_length(a.format, t, s, f.bytes);
    }
    const uint32_t end = block_inclusive_scan<kWaves>(len, part);
    if (i < n) a.ends[i] = end;
    if (threadIdx.x == kWireBlockFrames - 1) a.block[blockIdx.x] = end;
}

__global__ __launch_bounds__(kWireScanThreads) void wire_totals(const WireArgs a, uint32_t n_blocks)
{
    __shared__ uint32_t part[kWireScanThreads / 64];
    uint32_t carry = 0;
    for (uint32_t b0 = 0; b0 < n_blocks; b0 += kWireScanThreads) { // (uniform trip count: every thread meets the barriers)
        const uint32_t b = b0 + threadIdx.x;
        const uint32_t total = b < n_blocks ? a.block[b] : 0u;
        const uint32_t incl = block_inclusive_scan<kWireScanThreads / 64>(total, part);
        if (b < n_blocks) a.block[b] = carry + incl - total;
        if (threadIdx.x == kWireScanThreads - 1) part[0] = incl; // the round's sum, to every thread
        __syncthreads();
        carry += part[0];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        a.wire_hdr[0] = carry;
        a.wire_hdr[1] = list_count(a);
    }
}

__global__ __launch_bounds__(kWireBlockFrames) void wire_write(const WireArgs a)
{
    __shared__ uint32_t local_end[kWireBlockFrames];
    __shared__ uint32_t stage[kStageWords];
    const uint32_t n = list_count(a);
    const uint32_t first = blockIdx.x * kWireBlockFrames;
    if (first >= n) return; // (uniform)
    const uint32_t mine = n - first < kWireBlockFrames ? n - first : kWireBlockFrames;
    const uint32_t tid = threadIdx.x, i = first + tid;
    const uint32_t g0 = a.block[blockIdx.x]; // where this workgroup's span starts in the stream
    if (tid < mine) local_end[tid] = a.ends[i];
    __syncthreads();
    const uint32_t total = local_end[mine - 1];
    const uint32_t lead = g0 & 3u;          // stage byte j is stream byte (g0 - lead) + j
    uint8_t *image = reinterpret_cast<uint8_t *>(stage);
    if (tid < mine) {
        const uint32_t start = tid ? local_end[tid - 1] : 0u;
        const adsb_frame f = a.frames[i];
        uint64_t t;
        uint32_t s;
        frame_stamp(a, i, f, &t, &s);
        wire_encode(a.format, t, s, f.bytes, image + lead + start); // local_end[tid] - start bytes: wire_length's count
        a.ends[i] = g0 + local_end[tid];
    }
    __syncthreads();
    const uint32_t g1 = g0 + total;
    const uint32_t up = (g0 + 3u) & ~3u;
    const uint32_t body0 = up < g1 ? up : g1;                 // [g0, body0): bytes in front of the first aligned dword
    const uint32_t body1 = (g1 & ~3u) > body0 ? (g1 & ~3u) : body0; // [body0, body1): whole dwords; [body1, g1): the tail
    const uint32_t origin = g0 - lead;
    if (tid < body0 - g0) a.out[g0 + tid] = image[lead + tid];
    uint32_t *out32 = reinterpret_cast<uint32_t *>(a.out); // (a.out is dword-aligned: launch_wire checks)
    for (uint32_t w = (body0 >> 2) + tid; w < (body1 >> 2); w += kWireBlockFrames) out32[w] = stage[w - (origin >> 2)];
    if (tid < g1 - body1) a.out[body1 + tid] = image[body1 - origin + tid];
}

} // namespace

hipError_t launch_wire(hipStream_t s, const WireArgs &a)
{
    if (((uintptr_t)a.out & 3u) || (uint64_t)a.cap * kWireMaxBytes > 0xFFFFFFFFull) return hipErrorInvalidValue;
    const uint32_t blocks = wire_blocks(a.cap);
    if (blocks) hipLaunchKernelGGL(wire_lengths, dim3(blocks), dim3(kWireBlockFrames), 0, s, a);
    hipLaunchKernelGGL(wire_totals, dim3(1), dim3(kWireScanThreads), 0, s, a, blocks);
    if (blocks) hipLaunchKernelGGL(wire_write, dim3(blocks), dim3(kWireBlockFrames), 0, s, a);
    return hipGetLastError();
}

} // namespace adsbk
