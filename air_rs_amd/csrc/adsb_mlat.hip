// adsb_mlat.hip -- transmitter positions from correlated receptions (adsb_multilaterate / adsb_multilaterate_of,
// include/adsb_hip.h "Multilaterate"; adsb_mlat.h has the solver's text, shared with the CPU mirror).
//
// Two steps in stream order, nothing read back in between:
//   1 mlat_solve    16 lanes per message, four messages per wavefront, kMlatPerBlock = 16 per workgroup of 256 threads.
//                   Lane l of a message's 16 holds its receptions k = l (mod 16), at most 16 of them: a bit mask of
//                   the used ones, and the station and rho of the first (k = l) in registers -- all there is for a
//                   message of up to 16 receptions; the others are read again in every pass.  A pass adds the lane's
//                   range rows at one point into 15 partial sums and folds them with __shfl_xor(v, m, 16) for m = 8, 4,
//                   2, 1: the 16 lanes are one DPP row, no LDS and no barrier, and since a + b = b + a every lane ends
//                   with the same bits.  Everything after the fold (the altitude row, the 4 x 4 factorisation, the step
//                   rule) is computed by all 16 lanes alike, so every branch of the solver is uniform across a
//                   message's lanes; the four messages of a wavefront diverge from each other and only there.  Lane 0
//                   stores the fix.  The stations (32 bytes each, at most 256) are staged in LDS once per workgroup,
//                   with the kernel's one barrier, before any thread leaves.
//   2 reduce        (rocPRIM) of the fixes' flags into the header {n_messages, n_attempted, n_valid, flags}.
// No atomics, no workgroup waits for another.  Plain stores.
//
// Every index a thread forms, and its bound.  M, N: the lists' lengths (a.n_msgs, a.n_recs, or counts_dev[0], [1] clipped
// to them); R = a.n_receivers <= 256.
//   stations[i], lds[i]   i = threadIdx.x + 256 q < R
//   msgs[g], fixes[g]     g = blockIdx.x x 16 + threadIdx.x / 16, used only when g < M
//   recs[first + k]       k < n <= 256 only after first + n <= N was checked in 64 bits (else BAD_INDEX, nothing read)
//   lds[rec.receiver]     only after rec.receiver < R was checked for EVERY reception of the message (else BAD_INDEX)
//   rx[rec.frame]         TICKS only, only after rec.frame < a.n_rx was checked for every reception (else BAD_INDEX)
//   the reduction         fixes[i].flags for i < M
#include <hip/hip_runtime.h>

#include <cstring>

#include <rocprim/rocprim.hpp>

#include "adsb_kernels.h"
#include "adsb_mlat.h"

namespace adsbk {

namespace {

__device__ __forceinline__ double mlat_fold(double v)
{
#pragma clang fp contract(off)
    v = v + __shfl_xor(v, 8, kMlatLanes);
    v = v + __shfl_xor(v, 4, kMlatLanes);
    v = v + __shfl_xor(v, 2, kMlatLanes);
    v = v + __shfl_xor(v, 1, kMlatLanes);
    return v;
}

__device__ __forceinline__ uint32_t mlat_fold_u32(uint32_t v)
{
    v = v + (uint32_t)__shfl_xor((int)v, 8, kMlatLanes);
    v = v + (uint32_t)__shfl_xor((int)v, 4, kMlatLanes);
    v = v + (uint32_t)__shfl_xor((int)v, 2, kMlatLanes);
    v = v + (uint32_t)__shfl_xor((int)v, 1, kMlatLanes);
    return v;
}

// One lane's share of a message.
struct MlatLane {
    const adsb_reception *recs; // the message's first reception
    const adsb_wire_rx *rx;
    const MlatStation *st;      // the staged table
    MlatParams p;
    uint32_t n, lane, used;     // receptions of the message; bit j of used: reception lane + 16 j is used
    uint64_t t0;
    double clock0;
    double sx, sy, sz, rho;     // reception k = lane

    __device__ __forceinline__ uint64_t time_of(const adsb_reception &r) const
    {
        return p.time_source == ADSB_MLAT_TIME_TICKS ? rx[r.frame].ticks : r.time;
    }

    // the folded sums of the range rows at x
    __device__ __forceinline__ void operator()(const double *x, MlatSums &s) const
    {
        mlat_sums_zero(s);
        if (used & 1u) mlat_range_row(s, x, sx, sy, sz, rho);
        for (uint32_t j = 1, k = lane + kMlatLanes; k < n; ++j, k += kMlatLanes) {
            if (!(used >> j & 1u)) continue;
            const adsb_reception r = recs[k];
            const MlatStation q = st[r.receiver];
            mlat_range_row(s, x, q.x, q.y, q.z, mlat_rho(p, time_of(r), t0, q.clock, clock0));
        }
        for (int i = 0; i < 15; ++i) s.v[i] = mlat_fold(s.v[i]);
    }
};

__global__ __launch_bounds__(kMlatBlock) void mlat_solve(const MlatArgs a)
{
#pragma clang fp contract(off)
    __shared__ MlatStation lds[kMlatMaxReceivers];
    for (uint32_t i = threadIdx.x; i < a.n_receivers; i += kMlatBlock) lds[i] = a.stations[i];
    __syncthreads();

    uint32_t n_msgs = a.n_msgs, n_recs = a.n_recs;
    if (a.counts_dev) {
        const uint64_t m = a.counts_dev[0], r = a.counts_dev[1];
        n_msgs = m < n_msgs ? (uint32_t)m : n_msgs;
        n_recs = r < n_recs ? (uint32_t)r : n_recs;
    }
    const uint32_t g = blockIdx.x * kMlatPerBlock + threadIdx.x / kMlatLanes;
    const uint32_t lane = threadIdx.x % kMlatLanes;
    if (g >= n_msgs) return; // whole lane groups leave: the shuffles below stay inside a group

    const adsb_message msg = a.msgs[g];
    const uint32_t n = msg.n_receptions;
    adsb_mlat_fix fix;
    if ((uint64_t)msg.first + n > (uint64_t)n_recs) {
        fix = mlat_fix_empty(ADSB_MLAT_BAD_INDEX, 0);
    } else if (n > ADSB_MLAT_MAX_RECEPTIONS) {
        fix = mlat_fix_empty(ADSB_MLAT_TOO_MANY, 0);
    } else {
        MlatLane L;
        L.recs = a.recs + msg.first;
        L.rx = a.rx;
        L.st = lds;
        L.p = a.p;
        L.n = n;
        L.lane = lane;
        const bool ticks = a.p.time_source == ADSB_MLAT_TIME_TICKS;
        uint32_t bad = 0;
        for (uint32_t k = lane; k < n; k += kMlatLanes) {
            const adsb_reception r = L.recs[k];
            if (r.receiver >= a.n_receivers || (ticks && r.frame >= a.n_rx)) bad = 1;
        }
        if (mlat_fold_u32(bad)) {
            fix = mlat_fix_empty(ADSB_MLAT_BAD_INDEX, 0);
        } else {
            // the used mark: no earlier reception of the message has this one's receiver
            uint32_t used = 0;
            for (uint32_t j = 0, k = lane; k < n; ++j, k += kMlatLanes) {
                const uint32_t mine = L.recs[k].receiver;
                bool first = true;
                for (uint32_t e = 0; e < k; ++e) first = first && L.recs[e].receiver != mine;
                used |= (first ? 1u : 0u) << j;
            }
            L.used = used;
            const uint32_t n_used = mlat_fold_u32((uint32_t)__popc(used));
            double alt_m = 0.0;
            const bool has_alt = (a.p.flags & ADSB_MLAT_USE_ALTITUDE) && mlat_altitude_of(msg.bytes, alt_m);
            if (n_used < mlat_need(a.p, has_alt)) { // n = 0 ends here too
                fix = mlat_fix_empty(ADSB_MLAT_TOO_FEW, n_used);
            } else {
                const adsb_reception r0 = L.recs[0];
                const MlatStation q0 = lds[r0.receiver];
                L.t0 = L.time_of(r0);
                L.clock0 = q0.clock;
                L.sx = L.sy = L.sz = L.rho = 0.0;
                double cx = 0.0, cy = 0.0, cz = 0.0; // the centroid's partial sums, ascending k
                for (uint32_t j = 0, k = lane; k < n; ++j, k += kMlatLanes) {
                    if (!(used >> j & 1u)) continue;
                    const adsb_reception r = L.recs[k];
                    const MlatStation q = lds[r.receiver];
                    if (j == 0) {
                        L.sx = q.x;
                        L.sy = q.y;
                        L.sz = q.z;
                        L.rho = mlat_rho(a.p, L.time_of(r), L.t0, q.clock, L.clock0);
                    }
                    cx += q.x;
                    cy += q.y;
                    cz += q.z;
                }
                const double nu = (double)n_used;
                const double cen[3] = {mlat_fold(cx) / nu, mlat_fold(cy) / nu, mlat_fold(cz) / nu};
                const double s0[3] = {q0.x, q0.y, q0.z};
                fix = mlat_solve_message(a.p, n_used, has_alt, alt_m, s0, cen, L);
            }
        }
    }
    if (lane == 0) a.fixes[g] = fix;
}

// the header's reduction reads the flags of fix i, and nothing for i at or past the list's length
struct MlatCountAt {
    const adsb_mlat_fix *fixes;
    const uint64_t *counts_dev;
    uint32_t n_msgs;
    __device__ MlatCount operator()(uint32_t i) const
    {
        uint32_t m = n_msgs;
        if (counts_dev && counts_dev[0] < (uint64_t)m) m = (uint32_t)counts_dev[0];
        if (i >= m) return MlatCount{0, 0, 0, 0};
        return mlat_count_of(fixes[i].flags);
    }
};

struct MlatCountOp {
    __device__ MlatCount operator()(const MlatCount &x, const MlatCount &y) const { return mlat_count_add(x, y); }
};

static_assert(sizeof(MlatCount) == sizeof(adsb_mlat_header), "the reduction writes the header");

hipError_t mlat_reduce(hipStream_t st, const MlatArgs &a, void *temp, size_t &temp_bytes)
{
    return rocprim::reduce(temp, temp_bytes,
                           rocprim::make_transform_iterator(rocprim::counting_iterator<uint32_t>(0u),
                                                            MlatCountAt{a.fixes, a.counts_dev, a.n_msgs}),
                           reinterpret_cast<MlatCount *>(a.hdr), MlatCount{0, 0, 0, 0}, (size_t)a.n_msgs, MlatCountOp(), st);
}

} // namespace

size_t mlat_temp_bytes(size_t n_msgs)
{
    MlatArgs a{};
    a.n_msgs = (uint32_t)n_msgs;
    size_t need = 0;
    if (mlat_reduce((hipStream_t)0, a, nullptr, need) != hipSuccess) return 0;
    return need + 256;
}

hipError_t launch_mlat(hipStream_t st, const MlatArgs &a)
{
    if (a.n_msgs == 0) return hipMemsetAsync(a.hdr, 0, sizeof(adsb_mlat_header), st);
    if (a.n_receivers == 0 || a.n_receivers > kMlatMaxReceivers) return hipErrorInvalidValue;
    const uint32_t blocks = (uint32_t)(((uint64_t)a.n_msgs + kMlatPerBlock - 1) / kMlatPerBlock);
    hipLaunchKernelGGL(mlat_solve, dim3(blocks), dim3(kMlatBlock), 0, st, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    size_t tb = a.temp_bytes;
    return mlat_reduce(st, a, a.temp, tb);
}

} // namespace adsbk
