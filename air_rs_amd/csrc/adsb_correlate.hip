// adsb_correlate.hip -- a multi-receiver frame list as ONE de-duplicated, time-ordered message list with every
// message's receptions (adsb_correlate_launch / adsb_correlate_of, include/adsb_hip.h "Correlate"; adsb_correlate.h has
// the key compare, the head rule and the aggregate's combine, shared with the CPU mirror).
//
// Six steps in stream order, n known to the host before the first and nothing read back in between:
//   1 corr_keys     one thread per reception j: its receiver (binary search of j in the receivers' prefix), T, the two
//                   key words.
//   2 merge sort    (rocPRIM, one comparator sort) of the list indices into group order (K, T, j): ord[p] = j.  The
//                   order is total, so the result does not depend on how the sort splits its work.
//   3 scan          (rocPRIM inclusive_scan) of the per-reception aggregate in group order with corr_combine, whose
//                   head mark makes it a segmented scan: scan[p] = the aggregate of p's group up to p, first_t = the
//                   group's time.  The input (head rule included) is computed where the scan loads it.
//   4 radix sort    (rocPRIM, stable) of the positions p by the group's time scan[p].first_t.  Inside equal times the
//                   group order is kept, so the result is (time, K, T, j): every group contiguous, groups in message
//                   order.  It sorts all n receptions by a per-reception key: the group count is not needed.
//   5 scan          (rocPRIM inclusive_scan) of the heads in that order (a head: its aggregate counts one reception):
//                   midx[q] - 1 = the message of output position q.
//   6 corr_write    one thread per output position q: its adsb_reception; the last of a group (the next position is a
//                   head, or q = n - 1) holds the whole group's aggregate and writes the adsb_message and its
//                   adsb_frame; q = n - 1 writes the header.
// No atomics in these kernels, no workgroup waits for another, no thread loops over a group: the work is the two sorts'
// and two scans' whatever the groups' lengths.  Plain stores.  Everything a thread addresses: frames / levels / t / lo /
// hi / rx [j], ord / scan [p], pos / midx / head_t / recs [q], msgs / frames_out [m] with j, p, q, m < n; prefix[r + 1]
// and base[r] with r < n_receivers.
#include <hip/hip_runtime.h>

#include <cstring>

#include <rocprim/rocprim.hpp>

#include "adsb_correlate.h"
#include "adsb_kernels.h"

namespace adsbk {

namespace {

__global__ __launch_bounds__(kCorrBlock) void corr_keys(const CorrArgs a)
{
    const uint32_t j = blockIdx.x * kCorrBlock + threadIdx.x;
    if (j >= a.n) return;
    // the receiver r with prefix[r] <= j < prefix[r + 1] (prefix[n_receivers] = n > j; receivers without frames repeat)
    uint32_t lo = 0, hi = a.n_receivers - 1;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (a.prefix[mid + 1] > (uint64_t)j) hi = mid;
        else lo = mid + 1;
    }
    const adsb_frame f = a.frames[j];
    a.rx[j] = lo;
    a.t[j] = (a.base ? a.base[lo] : 0ull) + f.offset;
    a.lo[j] = corr_key_lo(f.bytes);
    a.hi[j] = corr_key_hi(f.bytes);
}

struct CorrLess {
    const uint64_t *t, *lo, *hi;
    __device__ CorrRec rec(uint32_t j) const { return CorrRec{t[j], lo[j], hi[j]}; }
    __device__ bool operator()(uint32_t ja, uint32_t jb) const { return corr_before(rec(ja), ja, rec(jb), jb); }
};

// the scan's input at group-order position p, computed where the scan loads it
struct CorrInput {
    CorrArgs a;
    __device__ CorrRec rec(uint32_t j) const { return CorrRec{a.t[j], a.lo[j], a.hi[j]}; }
    __device__ CorrAgg operator()(uint32_t p) const
    {
        const uint32_t j = a.ord[p];
        const CorrRec r = rec(j);
        const bool head = p == 0 || corr_is_head(rec(a.ord[p - 1]), r, a.window);
        return corr_agg_of(r.t, a.rx[j], a.frames[j], a.levels ? a.levels + j : nullptr, head);
    }
};

struct CorrOp {
    __device__ CorrAgg operator()(const CorrAgg &x, const CorrAgg &y) const { return corr_combine(x, y); }
};

struct CorrHeadTime {
    const CorrAgg *scan;
    __device__ uint64_t operator()(uint32_t p) const { return scan[p].first_t; }
};

// A reception is its group's head exactly when the aggregate up to it counts one reception.  (The aggregate's own
// head mark says that the run it covers contains a head, which holds for every prefix.)
__device__ __forceinline__ bool corr_head_at(const CorrAgg *scan, uint32_t p) { return scan[p].n == 1u; }

struct CorrHeadMark {
    const CorrAgg *scan;
    const uint32_t *pos;
    __device__ uint32_t operator()(uint32_t q) const { return corr_head_at(scan, pos[q]) ? 1u : 0u; }
};

__global__ __launch_bounds__(kCorrBlock) void corr_write(const CorrArgs a)
{
    const uint32_t q = blockIdx.x * kCorrBlock + threadIdx.x;
    if (q >= a.n) return;
    const uint32_t p = a.pos[q], j = a.ord[p];
    adsb_reception r;
    r.time = a.t[j];
    r.frame = j;
    r.receiver = (uint16_t)a.rx[j];
    r.reserved = 0;
    a.recs[q] = r;
    const bool last = q == a.n - 1;
    if (!last && !corr_head_at(a.scan, a.pos[q + 1])) return;
    const CorrAgg g = a.scan[p]; // the group's last reception: the whole group
    const uint32_t m = a.midx[q] - 1u;
    const adsb_frame f = a.frames[j];
    const adsb_message msg = corr_message_of(g, f.bytes, q + 1u - g.n);
    a.msgs[m] = msg;
    a.frames_out[m] = corr_frame_of(msg);
    if (last) {
        a.hdr[0] = (uint64_t)m + 1u;
        a.hdr[1] = a.n;
    }
}

using Count = rocprim::counting_iterator<uint32_t>;

} // namespace

// The four rocPRIM calls in order.  need != null: nothing is enqueued, *need = the most temporary storage any of them
// asks for at this n (a call given no storage only reports its size).
static hipError_t corr_primitives(hipStream_t st, const CorrArgs &a, size_t *need)
{
    const size_t n = a.n;
    void *temp = need ? nullptr : a.temp;
    size_t most = 0, tb = a.temp_bytes;
    hipError_t e = rocprim::merge_sort(temp, tb, Count(0u), a.ord, n, CorrLess{a.t, a.lo, a.hi}, st);
    if (e != hipSuccess) return e;
    most = tb > most ? tb : most;
    tb = a.temp_bytes;
    e = rocprim::inclusive_scan(temp, tb, rocprim::make_transform_iterator(Count(0u), CorrInput{a}), a.scan, n, CorrOp(),
                                st);
    if (e != hipSuccess) return e;
    most = tb > most ? tb : most;
    tb = a.temp_bytes;
    e = rocprim::radix_sort_pairs(temp, tb, rocprim::make_transform_iterator(Count(0u), CorrHeadTime{a.scan}), a.head_t,
                                  Count(0u), a.pos, n, 0, 64, st);
    if (e != hipSuccess) return e;
    most = tb > most ? tb : most;
    tb = a.temp_bytes;
    e = rocprim::inclusive_scan(temp, tb, rocprim::make_transform_iterator(Count(0u), CorrHeadMark{a.scan, a.pos}), a.midx,
                                n, rocprim::plus<uint32_t>(), st);
    if (e != hipSuccess) return e;
    most = tb > most ? tb : most;
    if (need) *need = most;
    return hipSuccess;
}

size_t corr_temp_bytes(size_t n)
{
    CorrArgs a{};
    a.n = (uint32_t)n;
    size_t need = 0;
    if (corr_primitives((hipStream_t)0, a, &need) != hipSuccess) return 0;
    return need + 256;
}

hipError_t launch_correlate(hipStream_t st, const CorrArgs &a)
{
    if (a.n == 0) return hipMemsetAsync(a.hdr, 0, 2 * sizeof(uint64_t), st);
    if (a.n_receivers == 0 || a.n_receivers > kCorrMaxReceivers) return hipErrorInvalidValue;
    const uint32_t blocks = (uint32_t)(((uint64_t)a.n + kCorrBlock - 1) / kCorrBlock);
    hipLaunchKernelGGL(corr_keys, dim3(blocks), dim3(kCorrBlock), 0, st, a);
    const hipError_t e = corr_primitives(st, a, nullptr);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(corr_write, dim3(blocks), dim3(kCorrBlock), 0, st, a);
    return hipGetLastError();
}

} // namespace adsbk
