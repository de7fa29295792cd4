// adsb_modes.hip -- the address of every frame of a list and the surveillance fields of Mode S replies (adsb_modes_of,
// include/adsb_hip.h "Mode S replies"; adsb_modes.h has the record of one frame and the known rule, shared with the CPU
// mirror).
//
// Seven steps in stream order, n and n_known_in known to the host before the first and nothing read back in between;
// m = n_known_in + n:
//   1 modes_frames   one thread per frame j: the 24 bytes, the syndrome (CRC-24 in the shift form over 4 or 11 bytes: the
//                    two loops unroll into straight VALU code with no table, no LDS and no indexed array, and the stage
//                    is bound by its 56 bytes of traffic per frame, not by them; finish_order's byte table would add an
//                    LDS fill and a barrier per workgroup to save what is already hidden), the record as far as the
//                    frame alone decides it, and the sort entry (address, 1 + j) of a SELF frame (2^24 for the others:
//                    they sort behind every address).  The same threads copy known_in's entries (address, 0) in front.
//   2 radix sort     (rocPRIM, stable, 25 key bits) of the m entries.  Stable: known_in's entry, then the SELF frames in
//                    list order, so the first entry of every run of equal addresses is the earliest.
//   3 scan           (rocPRIM inclusive_scan) of the heads of those runs: hidx[p] - 1 = the place in known_out.
//   4 modes_heads    one thread per sorted entry: a head writes known_out[k] and first[k]; the last entry n_known_out.
//   5 scan           (rocPRIM inclusive_scan) of the squitter marks (SELF with DF17/18, final since step 1) in list
//                    order: sidx[j] - 1 = the place in squitters.
//   6 modes_resolve  one thread per frame: an UNKNOWN record is looked up in known_out (binary search) and becomes KNOWN
//                    when first[k] <= j; a squitter's frame goes to its place; the workgroup's five kind counts (wave
//                    ballots, then LDS) go to tally[].
//   7 modes_totals   ONE workgroup: the header from tally[], squitter_counts[] from sidx[] at the receivers' ends.
// No atomics in these kernels, no workgroup waits for another (the dispatch boundaries are the only ordering), plain
// stores, and nothing depends on the grid: the same bytes from run to run.  Everything a thread addresses: frames / recs
// / sidx / squitters [j] with j < n (a squitter's place sidx[j] - 1 < n); known_in[i] with i < n_known_in; key / val /
// key_s / val_s / hidx [p] with p < m; known_out / first [k] with k < hidx[m - 1] <= m; tally[5 b + k] with b <
// modes_blocks(n), k < 5; prefix[r], prefix[r + 1] and sq_counts[r] with r < n_receivers <= 256.
#include <hip/hip_runtime.h>

#include <cstring>

#include <rocprim/rocprim.hpp>

#include "adsb_kernels.h"
#include "adsb_modes.h"

namespace adsbk {

namespace {

constexpr uint32_t kT = kModesBlock;
static_assert(kT % 64 == 0 && kT >= kModesMaxReceivers && kT >= 5, "whole waves, a thread per receiver and per kind");

__global__ __launch_bounds__(kT) void modes_frames(const ModesArgs a)
{
    const uint32_t j = blockIdx.x * kT + threadIdx.x;
    for (uint64_t i = j; i < a.n_known_in; i += (uint64_t)gridDim.x * kT) {
        a.key[i] = a.known_in[i];
        a.val[i] = 0u;
    }
    if (j >= a.n) return;
    const adsb_frame f = a.frames[j];
    const adsb_modes_rec r = modes_first(f.bytes);
    a.recs[j] = r;
    a.key[a.n_known_in + j] = modes_teaches(r) ? r.address : kModesNoAddress;
    a.val[a.n_known_in + j] = j + 1u;
}

__device__ __forceinline__ bool modes_head_at(const uint32_t *key_s, uint32_t p)
{
    const uint32_t k = key_s[p];
    return k < kModesNoAddress && (p == 0 || key_s[p - 1] != k);
}

struct ModesHeadMark {
    const uint32_t *key_s;
    __device__ uint32_t operator()(uint32_t p) const { return modes_head_at(key_s, p) ? 1u : 0u; }
};

struct ModesSquitterMark {
    const adsb_modes_rec *recs;
    __device__ uint32_t operator()(uint32_t j) const { return modes_is_squitter(recs[j]) ? 1u : 0u; }
};

__global__ __launch_bounds__(kT) void modes_heads(const ModesArgs a)
{
    const uint32_t m = a.n_known_in + a.n;
    const uint32_t p = blockIdx.x * kT + threadIdx.x;
    if (p >= m) return;
    if (modes_head_at(a.key_s, p)) {
        const uint32_t k = a.hidx[p] - 1u;
        a.known_out[k] = a.key_s[p];
        a.first[k] = a.val_s[p];
    }
    if (p == m - 1u) a.hdr->n_known_out = a.hidx[p];
}

__global__ __launch_bounds__(kT) void modes_resolve(const ModesArgs a)
{
    __shared__ uint32_t part[kT / 64][5];
    const uint32_t j = blockIdx.x * kT + threadIdx.x;
    uint32_t kind = 0xFFu; // no frame
    if (j < a.n) {
        adsb_modes_rec r = a.recs[j];
        if (r.kind == ADSB_MODES_UNKNOWN &&
            modes_is_known(a.known_out, a.first, (uint32_t)a.hdr->n_known_out, r.address, j)) {
            r.kind = ADSB_MODES_KNOWN;
            a.recs[j].kind = ADSB_MODES_KNOWN;
        }
        kind = r.kind;
        if (modes_is_squitter(r)) a.squitters[a.sidx[j] - 1u] = a.frames[j];
    }
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
    for (uint32_t k = 0; k < 5; ++k) {
        const uint32_t c = (uint32_t)__popcll(__ballot(kind == k));
        if (lane == 0) part[wave][k] = c;
    }
    __syncthreads();
    if (threadIdx.x < 5) {
        uint32_t s = 0;
#pragma unroll
        for (uint32_t w = 0; w < kT / 64; ++w) s += part[w][threadIdx.x];
        a.tally[5u * blockIdx.x + threadIdx.x] = s;
    }
}

__global__ __launch_bounds__(kT) void modes_totals(const ModesArgs a)
{
    __shared__ uint64_t part[kT / 64][5];
    const uint32_t blocks = modes_blocks(a.n);
    uint64_t s[5] = {0, 0, 0, 0, 0};
    for (uint32_t b = threadIdx.x; b < blocks; b += kT)
#pragma unroll
        for (uint32_t k = 0; k < 5; ++k) s[k] += a.tally[5u * b + k];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
    for (uint32_t k = 0; k < 5; ++k) {
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) s[k] += __shfl_down(s[k], d, 64);
        if (lane == 0) part[wave][k] = s[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t t[5] = {0, 0, 0, 0, 0};
        for (uint32_t w = 0; w < kT / 64; ++w)
            for (uint32_t k = 0; k < 5; ++k) t[k] += part[w][k];
        adsb_modes_header *h = a.hdr; // (n_known_out is modes_heads', or the 0 the launch cleared it to)
        h->n = a.n;
        h->n_self = t[ADSB_MODES_SELF];
        h->n_known = t[ADSB_MODES_KNOWN];
        h->n_unknown = t[ADSB_MODES_UNKNOWN];
        h->n_parity = t[ADSB_MODES_PARITY];
        h->n_unsupported = t[ADSB_MODES_UNSUPPORTED];
        h->n_squitters = a.n ? a.sidx[a.n - 1u] : 0u;
    }
    if (a.prefix && threadIdx.x < a.n_receivers) {
        const uint64_t lo = a.prefix[threadIdx.x], hi = a.prefix[threadIdx.x + 1u]; // lo <= hi <= n
        a.sq_counts[threadIdx.x] = (uint64_t)((hi ? a.sidx[hi - 1u] : 0u) - (lo ? a.sidx[lo - 1u] : 0u));
    }
}

using Count = rocprim::counting_iterator<uint32_t>;

} // namespace

// The three rocPRIM calls in order at n frames and m entries.  need != null: nothing is enqueued, *need = the most
// temporary storage any of them asks for (a call given no storage only reports its size).  between(): what runs
// between the sort's scan and the squitters' scan.
template <class F>
static hipError_t modes_primitives(hipStream_t st, const ModesArgs &a, size_t n, size_t m, size_t *need, F between)
{
    void *temp = need ? nullptr : a.temp;
    size_t most = 0, tb = a.temp_bytes;
    hipError_t e = hipSuccess;
    if (m) {
        e = rocprim::radix_sort_pairs(temp, tb, a.key, a.key_s, a.val, a.val_s, m, 0, kModesKeyBits, st);
        if (e != hipSuccess) return e;
        most = tb > most ? tb : most;
        tb = a.temp_bytes;
        e = rocprim::inclusive_scan(temp, tb, rocprim::make_transform_iterator(Count(0u), ModesHeadMark{a.key_s}), a.hidx, m,
                                    rocprim::plus<uint32_t>(), st);
        if (e != hipSuccess) return e;
        most = tb > most ? tb : most;
        tb = a.temp_bytes;
        between();
    }
    if (n) {
        e = rocprim::inclusive_scan(temp, tb, rocprim::make_transform_iterator(Count(0u), ModesSquitterMark{a.recs}), a.sidx,
                                    n, rocprim::plus<uint32_t>(), st);
        if (e != hipSuccess) return e;
        most = tb > most ? tb : most;
    }
    if (need) *need = most;
    return hipSuccess;
}

size_t modes_temp_bytes(size_t m)
{
    ModesArgs a{};
    size_t need = 0;
    if (modes_primitives((hipStream_t)0, a, m, m, &need, [] {}) != hipSuccess) return 0;
    return need + 256;
}

hipError_t launch_modes(hipStream_t st, const ModesArgs &a)
{
    if ((uint64_t)a.n + a.n_known_in > 0xFFFFFFFFull || (a.prefix && (a.n_receivers < 1 || a.n_receivers > kModesMaxReceivers)))
        return hipErrorInvalidValue;
    const uint32_t m = a.n_known_in + a.n;
    hipError_t e = hipMemsetAsync(a.hdr, 0, sizeof(adsb_modes_header), st);
    if (e != hipSuccess) return e;
    if (m) hipLaunchKernelGGL(modes_frames, dim3(a.n ? modes_blocks(a.n) : 1u), dim3(kT), 0, st, a);
    e = modes_primitives(st, a, a.n, m, nullptr,
                         [&] { hipLaunchKernelGGL(modes_heads, dim3(modes_blocks(m)), dim3(kT), 0, st, a); });
    if (e != hipSuccess) return e;
    if (a.n) hipLaunchKernelGGL(modes_resolve, dim3(modes_blocks(a.n)), dim3(kT), 0, st, a);
    hipLaunchKernelGGL(modes_totals, dim3(1), dim3(kT), 0, st, a);
    return hipGetLastError();
}

} // namespace adsbk
