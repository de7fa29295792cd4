// adsb_replies.hip -- Mode S replies from samples (adsb_replies_of, include/adsb_hip.h "Mode S replies from samples";
// adsb_replies.h has the text of one offset and of one frame, shared with the CPU mirror), and the merge of two frame
// lists (adsb_merge_lists_of).
//
// A scan of its own beside the demodulator's: it reads the samples and nothing of the demodulator's, and the
// demodulator's kernels know nothing of it.  Four steps in stream order, the tile count known to the host and nothing
// read back in between:
//   1 replies_scan   one workgroup per tile of T = 256 x R offsets (R = 32 for i8, 16 for CS16), tiles in the
//                    XCD-contiguous order of the demodulator's scan (a tile's halo is its neighbour's data).  The powers
//                    of T + 256 samples go to LDS (u16 for i8, u32 for CS16; one pad dword behind every 16, so that the
//                    256 runs start on different banks), from bounds-checked loads: samples past the channel read as
//                    zero, and the window rule, not the zeros, masks what they would give.  Thread t then slides over
//                    its run of R offsets with the sixteen powers of the window in registers: one LDS read, a min of
//                    four, a max of twelve and a compare per offset, the passes as bits of one word.  The rare passes
//                    (4! 12! / 16! = 1 in 1820 offsets of uniform noise; 1 in 955 of the bench's synthetic buffer, two
//                    to a wave) are decided one at a time by the whole wave: lane k compares the halves of frame bits
//                    k and 64 + k in LDS, two ballots are the frame, DF and the window rule are uniform, the syndrome
//                    is the XOR over the set bits of x^e mod G folded across the wave (adsb_replies.h,
//                    RepliesSynTable), then replies_decide with the binary search in known[].  A lane of its own per
//                    candidate would leave the 63 others waiting through its slice and CRC.
//                    What a thread keeps is one bit per offset of its run in one word.  The tile's seven counts go to
//                    tile[], and, only if it keeps a frame, its 256 words to bitmap[], all by plain stores.
//   2 replies_sums   one workgroup per 4096 tiles: the seven counts summed into group[].
//   3 replies_places one workgroup per 4096 tiles: the frames in front of its group (a sum over group[]), then the
//                    exclusive scan inside it: prefix[].  Workgroup 0 also writes the header, every byte of it.
//   4 replies_write  one workgroup per tile; all but the tiles that keep a frame end at once.  A prefix sum of the
//                    popcounts of the tile's 256 words ranks the kept offsets; each is sliced again by its wave, one
//                    bit per lane as in the scan but from the samples this time (an L2 hit), and written at prefix +
//                    rank if that is inside the capacity.  The first workgroups also write the per-channel counts
//                    from prefix[].
// No atomics, no workgroup waits for another (the dispatch boundary is the only ordering), plain stores, and nothing
// depends on the grid or the schedule: the same bytes from run to run, and EXACT: every kept offset has its bit.
// Everything a thread addresses: samples [s] with s < n_samples of its channel; tile[k n_tiles + i] with i < n_tiles, k
// < 7; bitmap[256 i + t]; group[k G + g] with g < G = replies_groups(n_tiles); prefix[i] with i <= n_tiles;
// frames[j] with j < cap; counts[c] with c < n_channels; the header.
//
// merge_lists: one thread per frame of either list; its place is its own index plus a binary search in the other
// list's segment of the same channel (replies_merge_place).
#include <hip/hip_runtime.h>

#include <type_traits>

#include "adsb_kernels.h"
#include "adsb_replies.h"

namespace adsbk {

namespace {

constexpr uint32_t kT = kRepliesThreads;
constexpr uint32_t kWaves = kT / 64;
constexpr uint32_t kW = kRepliesTileWords;
constexpr uint32_t kPerThread = kRepliesGroupTiles / kT; // tiles per thread of the folding kernels
static_assert(kRepliesGroupTiles % kT == 0 && kPerThread % 4 == 0, "whole uint4 of counts per thread");
static_assert(sizeof(adsb_frame) == 24, "three words per frame");

template <int ST>
struct Tile {
    using Pw = typename std::conditional<ST == ADSB_SAMPLE_I8, uint16_t, uint32_t>::type;
    static constexpr uint32_t kRun = replies_run(ST);
    static constexpr uint32_t kOffsets = replies_tile(ST);
    static constexpr uint32_t kSpan = kOffsets + 256;               // samples in LDS: the halo of 240, in whole chunks
    static constexpr uint32_t kPer = ST == ADSB_SAMPLE_I8 ? 8 : 4;  // samples per 16-byte chunk
    static constexpr uint32_t kChunks = kSpan / kPer;
    static constexpr uint32_t kFull = kChunks / kT;                 // chunks every thread loads
    static constexpr uint32_t kRow = 64 / sizeof(Pw);               // powers per 16 dwords
    static constexpr uint32_t kPad = 4 / sizeof(Pw);                // ... and per pad dword
    static constexpr uint32_t kLds = kSpan + kPad * (kSpan / kRow);
    static constexpr uint32_t kSampleBytes = ST == ADSB_SAMPLE_I8 ? 2 : 4;
    __device__ static constexpr uint32_t at(uint32_t k) { return k + kPad * (k / kRow); }
    static_assert(kRepliesHalo <= 256 && kRun <= 32 && kRun == kRow && kSpan % kPer == 0 && kRow % kPer == 0, "tile geometry");
};

static_assert(kRepliesAllCall == 2 && kRepliesParity == kRepliesTileWords - 1, "tile word k counts outcome k, from word 2 on");
__constant__ const RepliesSynTable kSyn = replies_syn_table();

template <int ST>
struct GlobalPower {
    const void *iq; // the channel's sample 0
    __device__ uint32_t operator()(uint64_t k) const { return replies_sample_power<ST>(iq, k); }
};

// the powers of one 16-byte chunk, as the dwords LDS takes
template <int ST>
__device__ __forceinline__ void chunk_powers(const uint4 v, uint32_t d[4])
{
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
        if (ST == ADSB_SAMPLE_I8) { // two samples per word: I0 Q0 I1 Q1
            const uint32_t p0 = (uint32_t)__builtin_amdgcn_sdot4((int)w[k], (int)(w[k] & 0xFFFFu), 0, false);
            const uint32_t p1 = (uint32_t)__builtin_amdgcn_sdot4((int)w[k], (int)(w[k] & 0xFFFF0000u), 0, false);
            d[k] = p0 | p1 << 16; // (<= 32768 each)
        } else {
            d[k] = replies_power((int16_t)(w[k] & 0xFFFFu), (int32_t)w[k] >> 16);
        }
    }
}
// ... to LDS: chunk q of the tile.  i8: eight u16 = four dwords; CS16: four dwords.  A chunk never straddles a pad.
template <int ST>
__device__ __forceinline__ void chunk_store(typename Tile<ST>::Pw *pw, uint32_t q, const uint32_t d[4])
{
    uint32_t *dst = reinterpret_cast<uint32_t *>(pw + Tile<ST>::at(q * Tile<ST>::kPer));
    dst[0] = d[0], dst[1] = d[1], dst[2] = d[2], dst[3] = d[3];
}
// a chunk at the ragged end of a channel: sample by sample, zero past the end
template <int ST>
__device__ __forceinline__ void chunk_edge(const void *chan, uint64_t s0, uint64_t n_samples, uint32_t d[4])
{
    uint32_t p[Tile<ST>::kPer];
#pragma unroll
    for (uint32_t e = 0; e < Tile<ST>::kPer; ++e) p[e] = s0 + e < n_samples ? replies_sample_power<ST>(chan, s0 + e) : 0u;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) d[k] = ST == ADSB_SAMPLE_I8 ? p[2 * k] | p[(2 * k + 1) % Tile<ST>::kPer] << 16 : p[k];
}

// the tile of workgroup b of n: eight contiguous ranges, one per XCD (adsb_kernels.hip, tile_of_workgroup, has the why)
__device__ __forceinline__ uint32_t replies_tile_of_workgroup(uint32_t b, uint32_t n)
{
    const uint32_t q = n >> 3, r = n & 7u, x = b & 7u, j = b >> 3;
    return x * q + (x < r ? x : r) + j;
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
    return v; // lane 0
}
// the sum of v over the lanes in front of this one, and *total over the workgroup; part: kWaves words of LDS
__device__ __forceinline__ uint64_t block_exclusive(uint64_t v, uint64_t *part, uint64_t *total)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint64_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t up = __shfl_up(inc, d, 64);
        if (lane >= (uint32_t)d) inc += up;
    }
    __syncthreads(); // part[] may still be read from an earlier call
    if (lane == 63) part[wave] = inc;
    __syncthreads();
    uint64_t before = 0, all = 0;
#pragma unroll
    for (uint32_t w = 0; w < kWaves; ++w) {
        before += w < wave ? part[w] : 0;
        all += part[w];
    }
    *total = all;
    return before + inc - v;
}

template <int ST>
__global__ __launch_bounds__(kT) void replies_scan(const RepliesArgs a)
{
    using G = Tile<ST>;
    __shared__ __attribute__((aligned(16))) typename G::Pw pw[G::kLds];
    __shared__ uint32_t part[kWaves][kW];
    __shared__ uint32_t syn[112];
    const uint32_t t = threadIdx.x;
    if (t < 112u) syn[t] = kSyn.r[t];
    const uint32_t tile = replies_tile_of_workgroup(blockIdx.x, a.n_tiles);
    const uint32_t chan = tile / a.tiles_per_channel;
    const uint64_t first = (uint64_t)(tile - chan * a.tiles_per_channel) * G::kOffsets; // the tile's first sample
    const char *iq = static_cast<const char *>(a.iq) + (size_t)G::kSampleBytes * a.channel_stride * chan;
    const uint64_t n = a.n_samples;

    // ---- the powers of [first, first + kSpan) into LDS
    if (first + G::kSpan <= n) { // (uniform) wholly inside the channel: every thread's loads are in flight together
        uint4 v[G::kFull];
#pragma unroll
        for (uint32_t m = 0; m < G::kFull; ++m)
            v[m] = *reinterpret_cast<const uint4 *>(iq + G::kSampleBytes * (first + (uint64_t)(t + m * kT) * G::kPer));
        uint4 tail = make_uint4(0, 0, 0, 0);
        const uint32_t q_tail = t + G::kFull * kT;
        if (q_tail < G::kChunks) tail = *reinterpret_cast<const uint4 *>(iq + G::kSampleBytes * (first + (uint64_t)q_tail * G::kPer));
#pragma unroll
        for (uint32_t m = 0; m < G::kFull; ++m) {
            uint32_t d[4];
            chunk_powers<ST>(v[m], d);
            chunk_store<ST>(pw, t + m * kT, d);
        }
        if (q_tail < G::kChunks) {
            uint32_t d[4];
            chunk_powers<ST>(tail, d);
            chunk_store<ST>(pw, q_tail, d);
        }
    } else {
        for (uint32_t q = t; q < G::kChunks; q += kT) {
            const uint64_t s0 = first + (uint64_t)q * G::kPer;
            uint32_t d[4];
            if (s0 + G::kPer <= n) chunk_powers<ST>(*reinterpret_cast<const uint4 *>(iq + G::kSampleBytes * s0), d);
            else chunk_edge<ST>(iq, s0, n, d);
            chunk_store<ST>(pw, q, d);
        }
    }
    __syncthreads();

    // ---- pre(i) over this thread's run: bit j of cand for offset first + t kRun + j
    const uint32_t base = t * G::kRun;
    uint32_t w[16];
#pragma unroll
    for (uint32_t k = 0; k < 15; ++k) w[k] = pw[G::at(base + k)];
    uint32_t cand = 0;
#pragma unroll
    for (uint32_t j = 0; j < G::kRun; ++j) {
        w[(j + 15u) & 15u] = pw[G::at(base + j + 15u)];
        uint32_t x[16];
#pragma unroll
        for (uint32_t k = 0; k < 16; ++k) x[k] = w[(j + k) & 15u];
        cand |= (uint32_t)replies_preamble16(x) << j;
    }
    // the window rule: offset i is examined iff i + kRepliesDfSpan <= n
    const uint64_t i0 = first + base;
    const uint64_t examined = i0 + kRepliesDfSpan <= n ? n - kRepliesDfSpan + 1u - i0 : 0u;
    if (examined < G::kRun) cand &= (1u << (uint32_t)examined) - 1u;

    // ---- the rare candidates, one at a time with the whole wave on each (a lane of its own per candidate would leave
    // the other 63 waiting through a slice and a CRC): lane k compares the two halves of frame bits k and 64 + k, two
    // ballots are the frame, and the syndrome is the XOR over the set bits of syn[place from the end].  Everything but
    // those compares is uniform over the wave, the counts included.
    const uint32_t lane = t & 63u, wave = t >> 6;
    const uint32_t high = lane < 48u ? lane : 0u; // (frame bits 64 + k exist for k < 48)
    uint32_t keep = 0, count[kW] = {0, 0, 0, 0, 0, 0, 0};
    for (;;) {
        const uint64_t busy = __ballot(cand != 0);
        if (!busy) break;
        const uint32_t src = (uint32_t)__ffsll((unsigned long long)busy) - 1u;
        const uint32_t word = (uint32_t)__builtin_amdgcn_readlane((int)cand, (int)src);
        const uint32_t j = (uint32_t)__ffs((int)word) - 1u;
        if (lane == src) cand &= cand - 1u;
        const uint32_t rel = (wave * 64u + src) * G::kRun + j; // the candidate's offset inside the tile
        const uint64_t i = first + rel;
        const uint32_t at0 = rel + 16u + 2u * lane, at1 = rel + 144u + 2u * high; // (at most rel + 239 < kSpan)
        const bool b_lo = pw[G::at(at0)] > pw[G::at(at0 + 1u)];
        const bool b_hi = pw[G::at(at1)] > pw[G::at(at1 + 1u)] && lane < 48u;
        const uint64_t w0 = __brevll(__ballot(b_lo)); // frame bit 0 in bit 63: ModesBytes::w0 of a long frame
        const uint32_t df = (uint32_t)(w0 >> 59);
        uint32_t o = kRepliesPreamble;
        if (replies_df_wanted(df) && i + 16u + 16u * modes_length(df) <= n) { // (uniform) 16 + 2 L samples
            uint32_t s = modes_length(df) == 7u ? (b_lo && lane < 56u ? syn[lane < 56u ? 55u - lane : 0u] : 0u)
                                                : (b_lo ? syn[111u - lane] : 0u) ^ (b_hi ? syn[47u - high] : 0u);
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) s ^= __shfl_xor(s, d, 64);
            o = replies_decide(df, (uint32_t)__builtin_amdgcn_readfirstlane((int)s), a.flags, a.known, a.n_known);
        }
        count[1] += 1;
#pragma unroll
        for (uint32_t k = kRepliesAllCall; k < kW; ++k) count[k] += o == k; // (tile word k counts outcome k)
        if (replies_kept(o)) {
            count[0] += 1;
            if (lane == src) keep |= 1u << j;
        }
    }

    // ---- the tile's counts, and its words if it keeps a frame
    if (lane == 0) {
#pragma unroll
        for (uint32_t k = 0; k < kW; ++k) part[wave][k] = count[k];
    }
    __syncthreads();
    uint32_t kept = 0;
#pragma unroll
    for (uint32_t v = 0; v < kWaves; ++v) kept += part[v][0];
    if (kept) a.bitmap[(size_t)kT * tile + t] = keep; // (uniform)
    if (t < kW) {
        uint32_t s = 0;
#pragma unroll
        for (uint32_t v = 0; v < kWaves; ++v) s += part[v][t];
        a.tile[(size_t)t * a.n_tiles + tile] = s;
    }
}

// group[k][g] = the sum of tile[k][...] over group g
__global__ __launch_bounds__(kT) void replies_sums(const RepliesArgs a)
{
    __shared__ uint32_t part[kWaves][kW];
    const uint32_t t = threadIdx.x, g = blockIdx.x, groups = gridDim.x;
    const uint64_t first = (uint64_t)g * kRepliesGroupTiles;
    uint32_t s[kW]; // (a group's offsets fit 32 bits: 4096 tiles of at most 8192)
#pragma unroll
    for (uint32_t k = 0; k < kW; ++k) s[k] = 0;
#pragma unroll 4
    for (uint32_t m = 0; m < kPerThread; ++m) {
        const uint64_t i = first + m * kT + t;
        if (i < a.n_tiles) {
#pragma unroll
            for (uint32_t k = 0; k < kW; ++k) s[k] += a.tile[(size_t)k * a.n_tiles + i];
        }
    }
    const uint32_t lane = t & 63u, wave = t >> 6;
#pragma unroll
    for (uint32_t k = 0; k < kW; ++k) {
        const uint32_t v = wave_sum(s[k]);
        if (lane == 0) part[wave][k] = v;
    }
    __syncthreads();
    if (t < kW) {
        uint32_t v = 0;
#pragma unroll
        for (uint32_t w = 0; w < kWaves; ++w) v += part[w][t];
        a.group[(size_t)t * groups + g] = v;
    }
}

// prefix[] of group g's tiles; workgroup 0: the header
__global__ __launch_bounds__(kT) void replies_places(const RepliesArgs a)
{
    __shared__ uint64_t part[kWaves];
    const uint32_t t = threadIdx.x, g = blockIdx.x, groups = gridDim.x;
    uint64_t total = 0;
    // frames in front of this group
    uint64_t mine = 0;
    for (uint32_t h = t; h < g; h += kT) mine += a.group[h];
    (void)block_exclusive(mine, part, &total);
    const uint64_t before_group = total;
    // the thread's kPerThread consecutive tiles
    const uint64_t first = (uint64_t)g * kRepliesGroupTiles + (uint64_t)t * kPerThread;
    uint32_t c[kPerThread];
#pragma unroll
    for (uint32_t m = 0; m < kPerThread; ++m) c[m] = first + m < a.n_tiles ? a.tile[first + m] : 0u;
    uint64_t sum = 0;
#pragma unroll
    for (uint32_t m = 0; m < kPerThread; ++m) sum += c[m];
    uint64_t at = before_group + block_exclusive(sum, part, &total);
#pragma unroll
    for (uint32_t m = 0; m < kPerThread; ++m) {
        if (first + m < a.n_tiles) a.prefix[first + m] = at;
        at += c[m];
    }
    if (g + 1u == groups && t == kT - 1u) a.prefix[a.n_tiles] = at; // (the last thread's tiles end the list)
    if (g != 0) return;
    // the header: the six counts over all groups
    uint64_t tot[kRepliesTallies];
#pragma unroll
    for (uint32_t k = 0; k < kRepliesTallies; ++k) {
        uint64_t v = 0;
        for (uint32_t h = t; h < groups; h += kT) v += a.group[(size_t)(k + 1u) * groups + h];
        uint64_t all;
        (void)block_exclusive(v, part, &all);
        tot[k] = all;
    }
    if (t == 0) replies_header_of(tot, a.cap, a.hdr);
}

template <int ST>
__global__ __launch_bounds__(kT) void replies_write(const RepliesArgs a)
{
    using G = Tile<ST>;
    __shared__ uint64_t part[kWaves];
    const uint32_t t = threadIdx.x, tile = blockIdx.x;
    // counts[]: frames of each channel inside the capacity
    const uint32_t c = tile * kT + t;
    if (tile < (a.n_channels + kT - 1u) / kT && c < a.n_channels) {
        const uint64_t lo = a.prefix[(size_t)c * a.tiles_per_channel], hi = a.prefix[(size_t)(c + 1u) * a.tiles_per_channel];
        a.counts[c] = (hi < a.cap ? hi : a.cap) - (lo < a.cap ? lo : a.cap);
    }
    if (a.tile[tile] == 0) return; // (uniform) nothing kept here: the common case
    const uint64_t place = a.prefix[tile];
    if (place >= a.cap) return;    // (uniform) wholly past the capacity
    uint32_t word = a.bitmap[(size_t)kT * tile + t];
    uint64_t total;
    uint64_t at = place + block_exclusive((uint64_t)__popc(word), part, &total); // where this thread's first frame goes
    const uint32_t chan = tile / a.tiles_per_channel;
    const uint64_t first = (uint64_t)(tile - chan * a.tiles_per_channel) * G::kOffsets;
    const GlobalPower<ST> p{static_cast<const char *>(a.iq) + (size_t)G::kSampleBytes * a.channel_stride * chan};
    const uint64_t n = a.n_samples;
    // one kept offset at a time with the whole wave on it, as in the scan: lane k compares the halves of frame bits k and
    // 64 + k, from the samples this time; a sample past the channel's end (behind a short frame) is not read
    const uint32_t lane = t & 63u, wave = t >> 6, high = lane < 48u ? lane : 0u;
    for (;;) {
        const uint64_t busy = __ballot(word != 0 && at < a.cap);
        if (!busy) break;
        const uint32_t src = (uint32_t)__ffsll((unsigned long long)busy) - 1u;
        const uint32_t w = (uint32_t)__builtin_amdgcn_readlane((int)word, (int)src);
        const uint64_t pos = (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)at, (int)src) |
                             (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(at >> 32), (int)src) << 32;
        const uint32_t j = (uint32_t)__ffs((int)w) - 1u;
        if (lane == src) word &= word - 1u, at += 1;
        const uint64_t i = first + (uint64_t)((wave * 64u + src) * G::kRun + j);
        const uint64_t s0 = i + 16u + 2u * lane, s1 = i + 144u + 2u * high;
        const bool b_lo = s0 + 1u < n && p(s0) > p(s0 + 1u);
        const uint64_t w0 = __brevll(__ballot(b_lo));
        ModesBytes b{w0 & ~0xFFull, 0};
        if (modes_length((uint32_t)(w0 >> 59)) == 14u) { // (uniform) a kept long frame: all of it is inside the channel
            const bool b_hi = lane < 48u && p(s1) > p(s1 + 1u);
            b = ModesBytes{w0, __brevll(__ballot(b_hi))};
        }
        const RepliesFrameWords f = replies_frame(a.offset_base + i, b);
        uint64_t *dst = reinterpret_cast<uint64_t *>(a.frames + pos);
        if (lane < 3u) dst[lane] = lane == 0u ? f.w[0] : lane == 1u ? f.w[1] : f.w[2];
    }
}

__global__ __launch_bounds__(kT) void merge_lists(const MergeArgs a)
{
    const uint64_t k = (uint64_t)blockIdx.x * kT + threadIdx.x;
    if (k >= (uint64_t)a.na + a.nb) return;
    const bool from_b = k >= a.na;
    const uint64_t j = from_b ? k - a.na : k;
    const uint64_t at = from_b ? replies_merge_place(a.b, a.prefix_b, a.a, a.prefix_a, a.n_channels, j, true)
                               : replies_merge_place(a.a, a.prefix_a, a.b, a.prefix_b, a.n_channels, j, false);
    const uint64_t *s = reinterpret_cast<const uint64_t *>(from_b ? a.b + j : a.a + j);
    uint64_t *d = reinterpret_cast<uint64_t *>(a.out + at);
    d[0] = s[0], d[1] = s[1], d[2] = s[2];
    if (a.src) a.src[at] = (uint32_t)j | (from_b ? ADSB_MERGE_FROM_B : 0u);
}

template <int ST>
hipError_t launch_replies_of(hipStream_t st, const RepliesArgs &a)
{
    const uint32_t groups = replies_groups(a.n_tiles);
    hipLaunchKernelGGL(replies_scan<ST>, dim3(a.n_tiles), dim3(kT), 0, st, a);
    hipLaunchKernelGGL(replies_sums, dim3(groups), dim3(kT), 0, st, a);
    hipLaunchKernelGGL(replies_places, dim3(groups), dim3(kT), 0, st, a);
    hipLaunchKernelGGL(replies_write<ST>, dim3(a.n_tiles), dim3(kT), 0, st, a);
    return hipGetLastError();
}

} // namespace

hipError_t launch_replies(hipStream_t st, int sample_type, const RepliesArgs &a)
{
    return sample_type == ADSB_SAMPLE_I8 ? launch_replies_of<ADSB_SAMPLE_I8>(st, a) : launch_replies_of<ADSB_SAMPLE_I16>(st, a);
}

hipError_t launch_merge_lists(hipStream_t st, const MergeArgs &a)
{
    const uint64_t n = (uint64_t)a.na + a.nb;
    if (n) hipLaunchKernelGGL(merge_lists, dim3((uint32_t)((n + kT - 1) / kT)), dim3(kT), 0, st, a);
    return hipGetLastError();
}

} // namespace adsbk
