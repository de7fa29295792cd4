// adsb_clock.hip -- receiver clock offsets and drift from position messages, and the corrected receptions
// (adsb_clock_sync / adsb_clock_sync_of / adsb_clock_apply, include/adsb_hip.h "Clock sync"; adsb_clock.h has the text
// shared with the CPU mirror).
//
// One pass, in stream order, nothing read back in between:
//   1 clock_rows      16 lanes per message, kClockPerBlock = 16 messages per workgroup of 256 threads, the stations
//                     (48 bytes each, at most 256) staged in LDS with the kernel's one barrier before any thread leaves.
//                     Every lane of a message decodes its position alike (uniform branches); lane l then writes the rows
//                     of the receptions k = l (mod 16) into the slots first + k: tau, y' and the pair key.  The keys were
//                     set to "empty" before, so every slot no row is written to stays empty.  One flag byte per message.
//   2 sort            (rocPRIM radix sort, 17 key bits, stable) of (key, slot): rows in (pair, slot) order, empty last.
//   3 clock_pairs     one wavefront per pair (lo < hi < R; R(R - 1) / 2 of them, none idle): the pair's run in the sorted keys by two binary searches,
//                     lane l adds its rows q = l (mod 64) in ascending q, the five sums fold with __shfl_xor for m = 32,
//                     16, 8, 4, 2, 1, lane 0 stores.  Every pair is written, the empty ones with zeros.
//   4 clock_solve     one workgroup: the edges as bit rows in LDS, the reached set by hop labels from the reference (one
//                     round per hop, at most R - 1), the unknowns' numbering, the normal equations into scratch, the
//                     left-looking L D Lt column by column (two barriers per column), the substitutions (one barrier per
//                     step), then the receivers' records and the header.  Once per list, not a throughput kernel.
// With cfg.max_residual_s > 0 a second pass: clock_residuals empties the keys of the rows to drop, then 2-4 again.
// clock_apply: 16 lanes per message over its receptions, the clocks staged in LDS.
// No atomics, no workgroup waits for another.  Plain stores.
//
// Every index a thread forms, and its bound.  M, N: the lists' lengths (a.n_msgs, a.n_recs, or counts_dev[0], [1] clipped
// to them); R = a.n_receivers <= 256; n = the unknowns <= 510.
//   stations[i], clocks[i], lds[i]   i = threadIdx.x + 256 q < R
//   msgs[g], msg_flags[g]  g < M; msgs[0] only by a thread that has a g < M
//   recs[first + k]        k < count only after first + count <= N was checked in 64 bits (else BAD_INDEX, nothing read)
//   lds[rec.receiver]      rows: only after rec.receiver < R was checked for EVERY reception of the message; apply: for
//                          that reception
//   rx[rec.frame]          TICKS only, after rec.frame < a.n_rx was checked likewise
//   tau, yp, key[first + k]  < N by the check above; key, key_sorted, slot_sorted[s] for s < a.n_recs (what was allocated)
//   tau, yp[slot_sorted[s]]  slot_sorted holds a permutation of 0 .. a.n_recs - 1
//   pairs[lo << 8 | hi]    lo, hi < 256: the arrays hold 65536 pairs
//   normal[i n + j]        i, j < n <= 510: the array holds 510 x 510
//   sol[r], hop[r], adj[r] r < R, or r a key's byte (< 256): the arrays hold 256
#include <hip/hip_runtime.h>

#include <cstring>

#include <rocprim/rocprim.hpp>

#include "adsb_clock.h"
#include "adsb_kernels.h"

namespace adsbk {

namespace {

__device__ __forceinline__ uint32_t clock_fold16_u32(uint32_t v)
{
    v = v + (uint32_t)__shfl_xor((int)v, 8, kClockLanes);
    v = v + (uint32_t)__shfl_xor((int)v, 4, kClockLanes);
    v = v + (uint32_t)__shfl_xor((int)v, 2, kClockLanes);
    v = v + (uint32_t)__shfl_xor((int)v, 1, kClockLanes);
    return v;
}

__device__ __forceinline__ double clock_fold(double v)
{
#pragma clang fp contract(off)
    for (uint32_t m = kClockPartials / 2; m; m >>= 1) v = v + __shfl_xor(v, (int)m, (int)kClockPartials);
    return v;
}

// the lists' lengths as the device knows them
__device__ __forceinline__ void clock_lengths(const ClockArgs &a, uint32_t &n_msgs, uint32_t &n_recs)
{
    n_msgs = a.n_msgs;
    n_recs = a.n_recs;
    if (a.counts_dev) {
        const uint64_t m = a.counts_dev[0], r = a.counts_dev[1];
        n_msgs = m < n_msgs ? (uint32_t)m : n_msgs;
        n_recs = r < n_recs ? (uint32_t)r : n_recs;
    }
}

__device__ __forceinline__ uint64_t clock_time_of(const ClockArgs &a, const adsb_reception &r)
{
    return a.p.time_source == ADSB_MLAT_TIME_TICKS ? a.rx[r.frame].ticks : r.time;
}

__global__ __launch_bounds__(kClockBlock) void clock_rows(const ClockArgs a)
{
#pragma clang fp contract(off)
    __shared__ ClockStation lds[kMlatMaxReceivers];
    for (uint32_t i = threadIdx.x; i < a.n_receivers; i += kClockBlock) lds[i] = a.stations[i];
    __syncthreads();

    uint32_t n_msgs, n_recs;
    clock_lengths(a, n_msgs, n_recs);
    const uint32_t g = blockIdx.x * kClockPerBlock + threadIdx.x / kClockLanes;
    const uint32_t lane = threadIdx.x % kClockLanes;
    if (g >= n_msgs) return; // whole lane groups leave: the shuffles below stay inside a group

    const adsb_message msg = a.msgs[g];
    const uint32_t n = msg.n_receptions;
    const bool ticks = a.p.time_source == ADSB_MLAT_TIME_TICKS;
    uint8_t flag = 0;
    if ((uint64_t)msg.first + n > (uint64_t)n_recs) {
        flag = kClockMsgBad;
    } else if (n <= ADSB_MLAT_MAX_RECEPTIONS) {
        const adsb_reception *recs = a.recs + msg.first;
        uint32_t bad = 0;
        for (uint32_t k = lane; k < n; k += kClockLanes) {
            const adsb_reception r = recs[k];
            if (r.receiver >= a.n_receivers || (ticks && r.frame >= a.n_rx)) bad = 1;
        }
        if (clock_fold16_u32(bad)) {
            flag = kClockMsgBad;
        } else {
            // the used mark: no earlier reception of the message has this one's receiver
            uint32_t used = 0;
            for (uint32_t j = 0, k = lane; k < n; ++j, k += kClockLanes) {
                const uint32_t mine = recs[k].receiver;
                bool first = true;
                for (uint32_t e = 0; e < k; ++e) first = first && recs[e].receiver != mine;
                used |= (first ? 1u : 0u) << j;
            }
            const uint32_t n_used = clock_fold16_u32((uint32_t)__popc(used));
            if (n_used >= 2) {
                const adsb_reception r0 = recs[0];
                const ClockStation q0 = lds[r0.receiver];
                double p[3];
                if (clock_position(a.p, q0, msg.bytes, p)) {
                    flag = kClockMsgEligible;
                    const uint64_t t0 = clock_time_of(a, r0);
                    const double tau = clock_tau(msg.time, a.msgs[0].time, a.p.seconds_per_time);
                    for (uint32_t j = 0, k = lane; k < n; ++j, k += kClockLanes) {
                        if (k == 0 || !(used >> j & 1u)) continue;
                        const adsb_reception r = recs[k];
                        const MlatStation q = lds[r.receiver].s;
                        const double y =
                            clock_row_y(a.p, mlat_dticks(a.p.time_source, clock_time_of(a, r), t0), q0.s, q, p);
                        double yp;
                        const uint32_t key = clock_key(r0.receiver, r.receiver, y, yp);
                        const uint32_t slot = msg.first + k;
                        a.tau[slot] = tau;
                        a.yp[slot] = yp;
                        a.key[slot] = key;
                    }
                }
            }
        }
    }
    if (lane == 0) a.msg_flags[g] = flag;
}

// wavefronts of clock_pairs for R receivers: R per two rows of pairs
__host__ __device__ inline uint32_t clock_pair_waves(uint32_t R)
{
    return R / 2u * R; // ceil((R - 1) / 2) x R
}

// first index in keys[0, n) whose key is not below `key`
__device__ __forceinline__ uint32_t clock_lower_bound(const uint32_t *keys, uint32_t n, uint32_t key)
{
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (keys[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(kClockBlock) void clock_pairs(const ClockArgs a, ClockPair *pairs)
{
#pragma clang fp contract(off)
    const uint32_t R = a.n_receivers;
    const uint32_t w = blockIdx.x * (kClockBlock / kClockPartials) + threadIdx.x / kClockPartials;
    const uint32_t lane = threadIdx.x % kClockPartials;
    // Row lo of the pairs has R - 1 - lo of them, so rows q and R - 2 - q together have R: wavefront w = q R + c takes
    // pair c of row q, or pair c - (R - 1 - q) of row R - 2 - q.  (R - 1) / 2 rows up, R(R - 1) / 2 pairs and no idle
    // wavefront but the second half of a middle row that is its own partner.
    if (w >= clock_pair_waves(R)) return; // whole wavefronts leave
    const uint32_t q = w / R, c = w % R, own = R - 1u - q;
    if (c >= own && R - 2u - q == q) return;
    const uint32_t lo = c < own ? q : R - 2u - q, hi = lo + 1u + (c < own ? c : c - own);
    const uint32_t key = clock_pair_at(lo, hi);
    const uint32_t begin = clock_lower_bound(a.key_sorted, a.n_recs, key);
    const uint32_t end = clock_lower_bound(a.key_sorted, a.n_recs, key + 1u);
    ClockPart part;
    clock_part_zero(part);
    for (uint32_t q = lane; q < end - begin; q += kClockPartials) {
        const uint32_t slot = a.slot_sorted[begin + q];
        clock_part_add(part, a.tau[slot], a.yp[slot]);
    }
    for (int i = 0; i < 5; ++i) part.v[i] = clock_fold(part.v[i]);
    if (lane == 0) {
        ClockPair o;
        o.st = part.v[0];
        o.stt = part.v[1];
        o.sy = part.v[2];
        o.sty = part.v[3];
        o.syy = part.v[4];
        o.n = end - begin;
        pairs[key] = o;
    }
}

// One solve of `stride` unknowns per receiver (2: offset and drift, 1: offset) for the `cnt` receivers rcv_of[].  The
// result is in v[]; false (for every thread alike): a pivot failed.
__device__ bool clock_solve_system(const ClockArgs &a, const ClockPair *pairs, const uint16_t *rcv_of, uint32_t cnt,
                                   uint32_t stride, double *d, double *v, uint32_t *fail)
{
#pragma clang fp contract(off)
    const uint32_t t = threadIdx.x, R = a.n_receivers, n = cnt * stride;
    double *m = a.normal;
    for (uint32_t e = t; e < n * n; e += kClockBlock) {
        const uint32_t i = e / n, j = e % n;
        if (j <= i)
            m[(size_t)i * n + j] =
                clock_normal_entry(a.p, pairs, R, rcv_of[i / stride], i % stride, rcv_of[j / stride], j % stride);
    }
    for (uint32_t i = t; i < n; i += kClockBlock) v[i] = clock_rhs_entry(a.p, pairs, R, rcv_of[i / stride], i % stride);
    if (t == 0) *fail = 0;
    __syncthreads();
    for (uint32_t j = 0; j < n; ++j) {
        // this thread's entries of column j: rows j + t and j + t + 256 (n <= 510)
        const uint32_t i0 = j + t, i1 = j + t + kClockBlock;
        double e0 = 0.0, e1 = 0.0;
        if (i0 < n) e0 = clock_ldl_entry(m, d, n, i0, j);
        if (i1 < n) e1 = clock_ldl_entry(m, d, n, i1, j);
        if (t == 0) {
            d[j] = e0;
            if (!clock_pivot_ok(e0, m[(size_t)j * n + j])) *fail = 1;
        }
        __syncthreads();
        if (*fail) break;
        const double dj = d[j];
        if (t != 0 && i0 < n) m[(size_t)i0 * n + j] = e0 / dj;
        if (i1 < n) m[(size_t)i1 * n + j] = e1 / dj;
        __syncthreads();
    }
    const bool failed = *fail != 0;
    __syncthreads(); // before the next solve clears it
    if (failed) return false;
    for (uint32_t k = 0; k < n; ++k) {
        const double vk = v[k];
        for (uint32_t i = k + 1 + t; i < n; i += kClockBlock) v[i] = v[i] - m[(size_t)i * n + k] * vk;
        __syncthreads();
    }
    for (uint32_t i = t; i < n; i += kClockBlock) v[i] = v[i] / d[i];
    __syncthreads();
    for (uint32_t k = n; k-- > 0;) {
        const double vk = v[k];
        for (uint32_t i = t; i < k; i += kClockBlock) v[i] = v[i] - m[(size_t)k * n + i] * vk;
        __syncthreads();
    }
    return true;
}

__global__ __launch_bounds__(kClockBlock) void clock_solve(const ClockArgs a, const ClockPair *pairs, const ClockPair *first)
{
#pragma clang fp contract(off)
    __shared__ uint32_t adj[kMlatMaxReceivers][8];
    __shared__ uint16_t hop[kMlatMaxReceivers], unk[kMlatMaxReceivers], rcv_of[kMlatMaxReceivers];
    __shared__ double d[kClockMaxUnknowns], v[kClockMaxUnknowns];
    __shared__ uint64_t red[4][kClockBlock];
    __shared__ uint32_t changed, fail, count;
    const uint32_t t = threadIdx.x, R = a.n_receivers;
    constexpr uint16_t kNone = 0xFFFFu;

    for (uint32_t w = 0; w < 8; ++w) {
        uint32_t bits = 0;
        if (t < R)
            for (uint32_t b = 0; b < 32; ++b) {
                const uint32_t o = w * 32 + b;
                if (o < R && clock_edge(a.p, pairs, t, o)) bits |= 1u << b;
            }
        adj[t][w] = bits;
    }
    hop[t] = t == a.p.reference ? (uint16_t)0 : kNone;
    __syncthreads();
    for (uint32_t round = 1; round < R; ++round) {
        if (t == 0) changed = 0;
        bool now = false;
        if (t < R && hop[t] == kNone)
            for (uint32_t w = 0; w < 8; ++w)
                for (uint32_t bits = adj[t][w]; bits; bits &= bits - 1u)
                    now = now || hop[w * 32 + (uint32_t)__ffs((int)bits) - 1u] != kNone;
        __syncthreads(); // every label was read before any is written
        if (now) {
            hop[t] = (uint16_t)round;
            changed = 1;
        }
        __syncthreads();
        const bool more = changed != 0;
        __syncthreads();
        if (!more) break;
    }
    if (t == 0) {
        uint32_t cnt = 0;
        for (uint32_t r = 0; r < R; ++r) {
            unk[r] = kNone;
            if (r != a.p.reference && hop[r] != kNone) {
                unk[r] = (uint16_t)cnt;
                rcv_of[cnt++] = (uint16_t)r;
            }
        }
        count = cnt;
    }
    __syncthreads();
    const uint32_t cnt = count;

    uint64_t hdr_flags = 0;
    uint32_t stride = (a.p.flags & ADSB_CLOCK_DRIFT) ? 2u : 1u;
    bool solved = clock_solve_system(a, pairs, rcv_of, cnt, stride, d, v, &fail);
    if (!solved && stride == 2u) {
        hdr_flags |= ADSB_CLOCK_HDR_DRIFT_DROPPED;
        stride = 1u;
        solved = clock_solve_system(a, pairs, rcv_of, cnt, stride, d, v, &fail);
    }
    if (!solved) hdr_flags |= ADSB_CLOCK_HDR_SINGULAR;

    if (t < R) {
        ClockSol s{0.0, 0.0};
        if (solved && unk[t] != kNone) {
            s.a = v[unk[t] * stride];
            if (stride == 2u) s.b = v[unk[t] * stride + 1u];
        }
        a.sol[t] = s;
    }
    __syncthreads();
    if (t < R)
        a.clocks[t] = clock_record(a.p, pairs, first, R, t, a.sol, a.stations[t].s.clock, hop[t] != kNone,
                                   solved && stride == 2u);

    // the header: integer sums, in any order
    uint32_t n_msgs, n_recs;
    clock_lengths(a, n_msgs, n_recs);
    uint64_t eligible = 0, bad = 0, rows = 0, kept = 0;
    for (uint32_t g = t; g < n_msgs; g += kClockBlock) {
        const uint8_t f = a.msg_flags[g];
        eligible += (f & kClockMsgEligible) ? 1 : 0;
        bad |= (f & kClockMsgBad) ? 1 : 0;
    }
    if (t < R)
        for (uint32_t hi = t + 1; hi < R; ++hi) {
            rows += first[clock_pair_at(t, hi)].n;
            kept += pairs[clock_pair_at(t, hi)].n;
        }
    red[0][t] = eligible;
    red[1][t] = bad;
    red[2][t] = rows;
    red[3][t] = kept;
    __syncthreads();
    if (t == 0) {
        uint64_t s[4] = {0, 0, 0, 0};
        for (uint32_t i = 0; i < kClockBlock; ++i) {
            s[0] += red[0][i];
            s[1] |= red[1][i];
            s[2] += red[2][i];
            s[3] += red[3][i];
        }
        adsb_clock_header h;
        h.n_messages = n_msgs;
        h.n_eligible = s[0];
        h.n_rows = s[2];
        h.n_dropped = s[2] - s[3];
        h.n_reached = cnt + 1u;
        h.flags = hdr_flags | (s[1] ? ADSB_CLOCK_HDR_BAD_INDEX : 0u);
        h.reserved[0] = h.reserved[1] = 0;
        *a.hdr = h;
    }
}

__global__ __launch_bounds__(kClockBlock) void clock_residuals(const ClockArgs a)
{
#pragma clang fp contract(off)
    const uint32_t s = blockIdx.x * kClockBlock + threadIdx.x;
    if (s >= a.n_recs) return;
    const uint32_t key = a.key[s];
    if (key > 0xFFFFu) return; // empty
    const double r = clock_residual(a.yp[s], a.tau[s], a.sol[key >> 8], a.sol[key & 0xFFu]);
    if (fabs(r) > a.p.max_residual_s) a.key[s] = kClockEmpty;
}

__global__ __launch_bounds__(kClockBlock) void clock_apply(const ClockArgs a)
{
#pragma clang fp contract(off)
    __shared__ double offset[kMlatMaxReceivers], drift[kMlatMaxReceivers];
    for (uint32_t i = threadIdx.x; i < a.n_receivers; i += kClockBlock) {
        offset[i] = a.clocks[i].offset_s;
        drift[i] = a.clocks[i].drift;
    }
    __syncthreads();

    uint32_t n_msgs, n_recs;
    clock_lengths(a, n_msgs, n_recs);
    const uint32_t g = blockIdx.x * kClockPerBlock + threadIdx.x / kClockLanes;
    const uint32_t lane = threadIdx.x % kClockLanes;
    if (g >= n_msgs) return;
    const adsb_message msg = a.msgs[g];
    const uint32_t n = msg.n_receptions;
    if ((uint64_t)msg.first + n > (uint64_t)n_recs) return;
    const bool ticks = a.p.time_source == ADSB_MLAT_TIME_TICKS;
    // the raw time everything is taken against: of the list's first reception, 0 if there is no such
    const adsb_message m0 = a.msgs[0];
    uint64_t ref = 0;
    if (m0.n_receptions && (uint64_t)m0.first + m0.n_receptions <= (uint64_t)n_recs) {
        const adsb_reception r = a.recs[m0.first];
        if (!ticks || r.frame < a.n_rx) ref = clock_time_of(a, r);
    }
    const double tau = clock_tau(msg.time, m0.time, a.p.seconds_per_time);
    for (uint32_t k = lane; k < n; k += kClockLanes) {
        const adsb_reception r = a.recs[msg.first + k];
        if (r.receiver >= a.n_receivers || (ticks && r.frame >= a.n_rx)) continue; // keeps its raw time
        const int64_t dt = mlat_dticks(a.p.time_source, clock_time_of(a, r), ref);
        a.corrected[msg.first + k].time =
            clock_apply_time(dt, offset[r.receiver], drift[r.receiver], tau, a.p.seconds_per_tick);
    }
}

hipError_t clock_sort(hipStream_t st, const ClockArgs &a, void *temp, size_t &temp_bytes)
{
    return rocprim::radix_sort_pairs(temp, temp_bytes, a.key, a.key_sorted, rocprim::counting_iterator<uint32_t>(0u),
                                     a.slot_sorted, (size_t)a.n_recs, 0u, kClockKeyBits, st);
}

hipError_t clock_pass(hipStream_t st, const ClockArgs &a, ClockPair *pairs)
{
    hipError_t e;
    if (a.n_recs) {
        size_t need = 0, tb = a.temp_bytes;
        if ((e = clock_sort(st, a, nullptr, need)) != hipSuccess) return e;
        if (need > tb) return hipErrorOutOfMemory; // the block was carved for at least this many receptions
        if ((e = clock_sort(st, a, a.temp, tb)) != hipSuccess) return e;
    }
    const uint32_t waves = clock_pair_waves(a.n_receivers), per = kClockBlock / kClockPartials;
    if (waves) { // one receiver has no pair
        hipLaunchKernelGGL(clock_pairs, dim3((waves + per - 1) / per), dim3(kClockBlock), 0, st, a, pairs);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(clock_solve, dim3(1), dim3(kClockBlock), 0, st, a, (const ClockPair *)pairs,
                       (const ClockPair *)a.pairs_first);
    return hipGetLastError();
}

} // namespace

size_t clock_temp_bytes(size_t n_recs)
{
    ClockArgs a{};
    a.n_recs = (uint32_t)n_recs;
    size_t need = 0;
    if (clock_sort((hipStream_t)0, a, nullptr, need) != hipSuccess) return 0;
    return need + 256;
}

hipError_t launch_clock_sync(hipStream_t st, const ClockArgs &a)
{
    if (a.n_receivers == 0 || a.n_receivers > kMlatMaxReceivers) return hipErrorInvalidValue;
    hipError_t e;
    if (a.n_recs && (e = hipMemsetAsync(a.key, 0xFF, sizeof(uint32_t) * a.n_recs, st)) != hipSuccess) return e;
    if (a.n_msgs) {
        const uint32_t blocks = (uint32_t)(((uint64_t)a.n_msgs + kClockPerBlock - 1) / kClockPerBlock);
        hipLaunchKernelGGL(clock_rows, dim3(blocks), dim3(kClockBlock), 0, st, a);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if ((e = clock_pass(st, a, a.pairs_first)) != hipSuccess) return e;
    if (a.p.max_residual_s > 0.0 && a.n_recs) {
        const uint32_t blocks = (uint32_t)(((uint64_t)a.n_recs + kClockBlock - 1) / kClockBlock);
        hipLaunchKernelGGL(clock_residuals, dim3(blocks), dim3(kClockBlock), 0, st, a);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        if ((e = clock_pass(st, a, a.pairs)) != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_clock_apply(hipStream_t st, const ClockArgs &a)
{
    if (a.n_recs == 0) return hipSuccess;
    hipError_t e = hipMemcpyAsync(a.corrected, a.recs, sizeof(adsb_reception) * a.n_recs, hipMemcpyDeviceToDevice, st);
    if (e != hipSuccess || a.n_msgs == 0) return e;
    const uint32_t blocks = (uint32_t)(((uint64_t)a.n_msgs + kClockPerBlock - 1) / kClockPerBlock);
    hipLaunchKernelGGL(clock_apply, dim3(blocks), dim3(kClockBlock), 0, st, a);
    return hipGetLastError();
}

} // namespace adsbk
