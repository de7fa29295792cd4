// adsb_wire_in.hip -- byte streams of Beast binary or AVR text back into ONE ordered frame list (adsb_wire_in_of,
// include/adsb_hip.h "Wire input"; adsb_wire_in.h has the reader of one mark, shared with the CPU mirror).
//
// Whether a 0x1A is a mark depends on the parity of the run of 0x1A bytes it ends, a run can be as long as the stream,
// and where a frame goes depends on every frame before it.  Both become local with one carried word per span.  The
// input is cut into spans of kWireInBlockBytes bytes, counted from the aligned dword that holds bytes[0] (so every load
// is a whole aligned dword; with a dword-aligned input a span is exactly that many stream bytes); kWireInThreads
// threads per span, 16 bytes each.  Six dispatches, in stream order:
//   1 wire_in_last    per span: the place of its last byte that is not 0x1A (dword loads, a maximum over the workgroup).
//   2 wire_in_carry   ONE workgroup: the running maximum of those over the spans, kWireInScanThreads at a time with a
//                     carry: in front of which byte the run that enters a span started.  Also clears the per-stream words.
//   3 wire_in_marks<false>  per span: the span plus a 43-byte halo staged in LDS (a mark in the span's last byte reads
//                     its whole frame from LDS), the streams' ends beside it.  Every thread turns its 16 bytes into bit
//                     masks (0x1A; a 0x1A followed by another byte; '*' or '@'), the last byte that is not 0x1A before
//                     any place comes from the mask, an exclusive maximum over the threads in front, or the span's
//                     carry, never further back than the start of the byte's own stream (a binary search over the ends
//                     for the thread's first byte, then forward).  An odd run ends in a mark; ONE lane reads it
//                     (wire_in_read), classifies and counts it.  The span's counters go to tally[], the stream's
//                     incomplete mark (its last mark: one writer) and the parity of the run it ends with (the thread that
//                     holds the stream's last byte: one writer) to inc[] and tail[].
//   4 wire_in_totals  ONE workgroup: the exclusive prefix of the spans' kept frames, the header, consumed[].
//   5 wire_in_marks<true>   the same walk again; a kept frame goes to its list index: the span's prefix plus an
//                     exclusive sum over the threads in front (a thread's 16 bytes hold at most one kept frame: complete
//                     frames do not overlap, a long one is 23 bytes or more and a short one, emitted with
//                     ADSB_WIRE_IN_SHORT, 16 or more).  Frames, rx and levels are written here.
//   6 wire_in_counts  ONE workgroup: counts[] by two binary searches per receiver over rx[].receiver, which ascends.
// No atomics, no workgroup waits for another (the dispatch boundaries are the only ordering), and nothing depends on the
// grid: the lists are the same bytes from run to run.  Hostile density (1A 33 1A 33 ...: a mark every 2 bytes, each cut
// by the next) costs a thread 8 short reads; at most one kept frame exists per 23 bytes (16 with short frames).
//
// Everything a thread addresses:
//   words[w]      w < ceil((lead + n_bytes) / 4): only dwords that hold at least one byte of the input are loaded (an
//                 aligned dword does not cross a page, so the up to 3 bytes beside the input are readable; they are
//                 masked to 0 and never parsed).
//   image[p]      (LDS) p < kWireInBlockBytes + 44 when staged; a reader reads p < limit <= kWireInBlockBytes + 44 and
//                 a mark at l < kWireInBlockBytes needs at most l + 43.
//   ends_l[r]     (LDS) r < n_streams: a byte g of the input has g < n_bytes = ends[n_streams - 1], so the forward walk
//                 `while (ends_l[r] <= g) ++r` stops at an r < n_streams; the tail walk checks r < n_streams itself.
//   last[b], carry[b], tally[b]   b < n_spans (the grid of 1, 3 and 5 is n_spans; 2 and 4 check b < n_spans).
//   inc[r], tail[r], counts[r], consumed[r]   r < n_streams <= 256.
//   frames[i], rx[i], levels[i]   i < cap, checked at the store.  rx[i] is read in 6 for i < n_frames <= cap.
#include "adsb_kernels.h"
#include "adsb_wire_in.h"

namespace adsbk {

namespace {

constexpr uint32_t kB = kWireInBlockBytes, kT = kWireInThreads, kS = kWireInScanThreads;
constexpr uint32_t kImageBytes = kB + kWireInHalo + 1; // the halo, and the byte that rounds it to whole dwords
constexpr uint32_t kImageWords = kImageBytes / 4;
static_assert(kImageBytes % 4 == 0 && kT % 64 == 0 && kS % 64 == 0 && kT >= kWireInMaxStreams && kS >= kWireInMaxStreams,
              "whole dwords, whole waves, a thread per stream");

struct OpSum {
    template <class T> __device__ T operator()(T a, T b) const { return a + b; }
};
struct OpMax {
    template <class T> __device__ T operator()(T a, T b) const { return a > b ? a : b; }
};

// Inclusive scan of v (identity 0) across a workgroup of W waves; *excl: the same without the thread's own v.  part: W
// words of LDS.  Every thread of the workgroup calls it.
template <uint32_t W, class T, class Op>
__device__ __forceinline__ T block_scan(T v, T *part, Op op, T *excl)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T o = __shfl_up(v, d, 64);
        if (lane >= (uint32_t)d) v = op(v, o);
    }
    if (lane == 63) part[wave] = v;
    __syncthreads();
    T before = 0;
#pragma unroll
    for (uint32_t w = 0; w < W; ++w) before = w < wave ? op(before, part[w]) : before;
    __syncthreads(); // part[] may be written again by the caller's next round
    const T prev = __shfl_up(v, 1, 64);
    *excl = lane ? op(before, prev) : before;
    return op(before, v);
}

// the last thread's inclusive value to every thread; one: a word of LDS
template <uint32_t N, class T>
__device__ __forceinline__ T block_last(T incl, T *one)
{
    if (threadIdx.x == N - 1) *one = incl;
    __syncthreads();
    const T all = *one;
    __syncthreads();
    return all;
}

// dword w of the input's aligned image with the bytes that are not the input's set to 0; 0 for a dword with none
__device__ __forceinline__ uint32_t load_word(const WireInArgs &a, uint32_t w)
{
    const uint64_t q = 4ull * w, end = (uint64_t)a.lead + a.n_bytes;
    if (q >= end) return 0u;
    uint32_t v = a.words[w];
    if (w == 0 && a.lead) v &= 0xFFFFFFFFu << (8u * a.lead);
    if (end - q < 4u) v &= 0xFFFFFFFFu >> (8u * (4u - (uint32_t)(end - q)));
    return v;
}

// bit k: byte k of v equals c
__device__ __forceinline__ uint32_t eq_mask(uint32_t v, uint32_t c)
{
    uint32_t m = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) m |= (((v >> (8u * k)) & 0xFFu) == c ? 1u : 0u) << k;
    return m;
}

__global__ __launch_bounds__(kT) void wire_in_last(const WireInArgs a)
{
    __shared__ uint32_t part[kT / 64], one;
    uint32_t best = 0;
#pragma unroll
    for (uint32_t k = 0; k < kB / 4 / kT; ++k) { // consecutive lanes, consecutive dwords
        const uint32_t w = k * kT + threadIdx.x;
        const uint32_t non = ~eq_mask(load_word(a, blockIdx.x * (kB / 4) + w), 0x1Au) & 0xFu;
        if (non) best = 4u * w + (31u - (uint32_t)__clz(non)) + 1u; // (w ascends with k)
    }
    uint32_t excl;
    const uint32_t all = block_last<kT>(block_scan<kT / 64>(best, part, OpMax(), &excl), &one);
    if (threadIdx.x == 0) a.last[blockIdx.x] = all;
}

__global__ __launch_bounds__(kS) void wire_in_carry(const WireInArgs a)
{
    __shared__ uint64_t part[kS / 64], one;
    if (threadIdx.x < a.n_streams) {
        const uint32_t r = threadIdx.x;
        a.inc[r] = 0u;
        a.tail[r] = a.ends[r] - (r ? a.ends[r - 1] : 0u); // a stream that ends in no 0x1A, or an empty one
    }
    uint64_t carry = 0;
    for (uint32_t b0 = 0; b0 < a.n_spans; b0 += kS) { // (uniform trip count: every thread meets the barriers)
        const uint32_t b = b0 + threadIdx.x;
        const uint32_t l = b < a.n_spans ? a.last[b] : 0u;
        const uint64_t v = l ? (uint64_t)b * kB + l : 0ull;
        uint64_t excl;
        const uint64_t incl = block_scan<kS / 64>(v, part, OpMax(), &excl);
        if (b < a.n_spans) a.carry[b] = excl > carry ? excl : carry;
        const uint64_t all = block_last<kS>(incl, &one);
        carry = all > carry ? all : carry;
    }
}

template <bool kWrite>
__global__ __launch_bounds__(kT) void wire_in_marks(const WireInArgs a)
{
    __shared__ uint32_t image[kImageWords];
    __shared__ uint32_t ends_l[kWireInMaxStreams];
    __shared__ uint32_t part[kT / 64], one;
    const uint32_t tid = threadIdx.x;
    for (uint32_t w = tid; w < kImageWords; w += kT) image[w] = load_word(a, blockIdx.x * (kB / 4) + w);
    if (tid < a.n_streams) ends_l[tid] = a.ends[tid];
    __syncthreads();
    const uint8_t *img = reinterpret_cast<const uint8_t *>(image);
    const bool beast = a.format == ADSB_WIRE_BEAST;
    const uint64_t base = (uint64_t)blockIdx.x * kB, in_end = (uint64_t)a.lead + a.n_bytes;
    const uint32_t l0 = 16u * tid;

    // the thread's 16 bytes and the one behind them as masks
    const uint4 v = reinterpret_cast<const uint4 *>(image)[tid];
    const uint32_t next = image[4u * tid + 4u];
    const uint32_t is1a = eq_mask(v.x, 0x1Au) | eq_mask(v.y, 0x1Au) << 4 | eq_mask(v.z, 0x1Au) << 8 |
                          eq_mask(v.w, 0x1Au) << 12 | (eq_mask(next, 0x1Au) & 1u) << 16;
    const uint32_t non = ~is1a & 0xFFFFu;
    uint32_t cand;
    if (beast) {
        cand = is1a & ~(is1a >> 1) & 0xFFFFu;
    } else {
        cand = (eq_mask(v.x, '*') | eq_mask(v.x, '@')) | (eq_mask(v.y, '*') | eq_mask(v.y, '@')) << 4 |
               (eq_mask(v.z, '*') | eq_mask(v.z, '@')) << 8 | (eq_mask(v.w, '*') | eq_mask(v.w, '@')) << 12;
    }
    uint32_t before; // 1 + the place in the span of the last byte that is not 0x1A in the threads in front; 0: none
    block_scan<kT / 64>(non ? l0 + (31u - (uint32_t)__clz(non)) + 1u : 0u, part, OpMax(), &before);
    const uint64_t carry = a.carry[blockIdx.x];
    // 1 + (lead + position) of the last byte that is not 0x1A in front of place l0 + j, stream starts aside
    const auto run_start = [&](uint32_t j) -> uint64_t {
        const uint32_t below = non & ((1u << j) - 1u);
        return below ? base + l0 + (31u - (uint32_t)__clz(below)) + 1u : before ? base + before : carry;
    };

    WireInTally tally{};
    WireInMark mine{};
    uint32_t mine_pos = 0, mine_rx = 0;
    bool have = false;
    const uint64_t q0 = base + l0;
    if (q0 < in_end) { // (else: nothing of the input in these 16 bytes; the masks are 0)
        const uint32_t g0 = q0 < a.lead ? 0u : (uint32_t)(q0 - a.lead);
        uint32_t r = 0, hi = a.n_streams - 1u; // the first stream that ends behind g0: g0 < n_bytes = the last end
        while (r < hi) {
            const uint32_t mid = (r + hi) >> 1;
            if (ends_l[mid] > g0) hi = mid;
            else r = mid + 1u;
        }
        if (beast && !kWrite) { // streams whose last byte is one of mine: the parity of the run they end with
            for (uint32_t t = r; t < a.n_streams && (uint64_t)ends_l[t] + a.lead <= q0 + 16u; ++t) {
                const uint32_t s0 = t ? ends_l[t - 1] : 0u, s1 = ends_l[t];
                if (s1 == s0 || (uint64_t)s1 - 1u + a.lead < q0) continue; // empty, or its last byte is in front of mine
                const uint32_t j = (uint32_t)((uint64_t)s1 - 1u + a.lead - q0); // < 16
                if (!(is1a >> j & 1u)) continue;                               // tail[t] is the stream's length already
                uint64_t rs = run_start(j);
                const uint64_t s0q = (uint64_t)s0 + a.lead;
                rs = rs < s0q ? s0q : rs;
                a.tail[t] = wire_in_tail(s1 - s0, (uint32_t)(q0 + j - rs) + 1u);
            }
        }
        while (cand) {
            const uint32_t j = (uint32_t)__ffs((int)cand) - 1u;
            cand &= cand - 1u;
            const uint32_t l = l0 + j;
            const uint64_t q = base + l;
            const uint32_t g = (uint32_t)(q - a.lead); // a byte of the input: bytes beside it are 0 and no candidate
            while (ends_l[r] <= g) ++r;
            const uint32_t s0 = r ? ends_l[r - 1] : 0u, s1 = ends_l[r];
            if (beast) {
                if (g + 1u >= s1) continue; // the run reaches the end of the stream: no mark
                uint64_t rs = run_start(j);
                const uint64_t s0q = (uint64_t)s0 + a.lead;
                rs = rs < s0q ? s0q : rs;
                if ((q - rs) & 1ull) continue; // an even run
            }
            const uint64_t room = (uint64_t)s1 + a.lead - base; // the stream's end as a place in the image
            const uint32_t limit = room < kImageBytes ? (uint32_t)room : kImageBytes;
            const WireInMark m = wire_in_read(beast, img, l, limit);
            const bool keep = wire_in_count(m, a.filter, &tally);
            if (!kWrite && m.state == kWinIncomplete) a.inc[r] = g - s0 + 1u;
            if (keep) {
                mine = m;
                mine_pos = g - s0;
                mine_rx = r;
                have = true;
            }
        }
    }

    uint32_t at; // kept frames of the span in front of this thread's
    const uint32_t kept = block_scan<kT / 64>(tally.kept, part, OpSum(), &at);
    if (!kWrite) {
        uint32_t x;
        WireInTally t{};
        t.kept = block_last<kT>(kept, &one);
        t.marks = block_last<kT>(block_scan<kT / 64>(tally.marks, part, OpSum(), &x), &one);
        t.cut = block_last<kT>(block_scan<kT / 64>(tally.cut, part, OpSum(), &x), &one);
        t.unknown = block_last<kT>(block_scan<kT / 64>(tally.unknown, part, OpSum(), &x), &one);
        t.other = block_last<kT>(block_scan<kT / 64>(tally.other, part, OpSum(), &x), &one);
        t.rejected = block_last<kT>(block_scan<kT / 64>(tally.rejected, part, OpSum(), &x), &one);
        if (tid == 0) a.tally[blockIdx.x] = t;
    } else {
        const uint64_t i = (uint64_t)a.tally[blockIdx.x].kept + at;
        if (have && i < a.cap) {
            a.frames[i] = wire_in_frame(mine, a.tick_bias);
            a.rx[i] = wire_in_rx(mine, mine_pos, mine_rx);
            if (a.levels) a.levels[i] = wire_in_level(mine.signal, a.sample_type);
        }
    }
}

__global__ __launch_bounds__(kS) void wire_in_totals(const WireInArgs a)
{
    __shared__ uint32_t part[kS / 64], one;
    __shared__ uint64_t part64[kS / 64], one64;
    uint64_t carry = 0, sums[5] = {0, 0, 0, 0, 0};
    for (uint32_t b0 = 0; b0 < a.n_spans; b0 += kS) { // (uniform trip count: every thread meets the barriers)
        const uint32_t b = b0 + threadIdx.x;
        WireInTally t{};
        if (b < a.n_spans) t = a.tally[b];
        uint32_t excl;
        const uint32_t incl = block_scan<kS / 64>(t.kept, part, OpSum(), &excl);
        // (fewer than 2^32 / 23 frames exist: the prefix fits 32 bits)
        if (b < a.n_spans) a.tally[b].kept = (uint32_t)carry + excl;
        carry += block_last<kS>(incl, &one);
        sums[0] += t.marks, sums[1] += t.cut, sums[2] += t.unknown, sums[3] += t.other, sums[4] += t.rejected;
    }
    uint64_t total[5];
#pragma unroll
    for (uint32_t k = 0; k < 5; ++k) {
        uint64_t x;
        total[k] = block_last<kS>(block_scan<kS / 64>(sums[k], part64, OpSum(), &x), &one64);
    }
    if (threadIdx.x == 0) {
        adsb_wire_in_header h{};
        h.n_frames = carry < a.cap ? carry : a.cap;
        h.total_found = carry;
        h.n_marks = total[0], h.n_cut = total[1], h.n_unknown = total[2], h.n_other = total[3], h.n_rejected = total[4];
        h.flags = carry > a.cap ? ADSB_FLAG_TRUNCATED : 0u;
        *a.hdr = h;
    }
    if (threadIdx.x < a.n_streams) {
        const uint32_t r = threadIdx.x, inc = a.inc[r];
        a.consumed[r] = inc ? inc - 1u : a.tail[r];
    }
}

__global__ __launch_bounds__(kS) void wire_in_counts(const WireInArgs a)
{
    if (threadIdx.x >= a.n_streams) return;
    const uint32_t n = (uint32_t)a.hdr->n_frames; // <= cap
    uint32_t first[2];                            // the first list index whose receiver is at least r, r + 1
#pragma unroll
    for (uint32_t k = 0; k < 2; ++k) {
        uint32_t lo = 0, hi = n;
        while (lo < hi) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (a.rx[mid].receiver >= threadIdx.x + k) hi = mid;
            else lo = mid + 1u;
        }
        first[k] = lo;
    }
    a.counts[threadIdx.x] = first[1] - first[0];
}

} // namespace

hipError_t launch_wire_in(hipStream_t s, const WireInArgs &a)
{
    if (((uintptr_t)a.words & 3u) || a.lead > 3u || a.n_streams < 1 || a.n_streams > kWireInMaxStreams ||
        a.n_spans != wire_in_spans((uint64_t)a.lead + a.n_bytes))
        return hipErrorInvalidValue;
    if (a.n_spans) hipLaunchKernelGGL(wire_in_last, dim3(a.n_spans), dim3(kT), 0, s, a);
    hipLaunchKernelGGL(wire_in_carry, dim3(1), dim3(kS), 0, s, a);
    if (a.n_spans) hipLaunchKernelGGL(wire_in_marks<false>, dim3(a.n_spans), dim3(kT), 0, s, a);
    hipLaunchKernelGGL(wire_in_totals, dim3(1), dim3(kS), 0, s, a);
    if (a.n_spans) hipLaunchKernelGGL(wire_in_marks<true>, dim3(a.n_spans), dim3(kT), 0, s, a);
    hipLaunchKernelGGL(wire_in_counts, dim3(1), dim3(kS), 0, s, a);
    return hipGetLastError();
}

} // namespace adsbk
