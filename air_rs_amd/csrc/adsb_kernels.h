// adsb_kernels.h -- launch interface between the C-ABI layer (adsb_api.cpp and the features' adsb_*_api.cpp) and the
// gfx950 kernels (adsb_kernels.hip, adsb_track.hip, adsb_levels.hip, ...).  Internal; the public boundary is
// include/adsb_hip.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/adsb_hip.h"
#include "adsb_mlat.h"
#include "adsb_clock_records.h"

namespace adsbk {

// ---- tiling constants (see DESIGN.md "Data layout") ---------------------------------------
#ifndef ADSB_KRUN
#define ADSB_KRUN 32
#endif
#ifndef ADSB_THREADS
#define ADSB_THREADS 256
#endif
constexpr int kThreads = ADSB_THREADS; // 4 waves per workgroup (a multiple of 64; the tile length scales with it)
constexpr int kRun = ADSB_KRUN; // consecutive offsets one lane slides over, per packed half (<= 64)
constexpr int kTile = 2 * kThreads * kRun; // offsets owned by one workgroup (16384 at kRun 32)
constexpr int kHalo = 256;      // >= 239 extra samples so PPM never leaves the tile; 16-aligned
constexpr int kMag = kTile + kHalo;
// CS16 keeps u16 magnitudes in LDS.  Runs of 16 offsets = 8192-offset tiles, 19 KB: the kernel's 85 VGPRs then allow
// five workgroups per CU (20 waves) where 16384-offset tiles (35 KB) allowed four -- and the finer tiles overlap better:
// 0.177 -> 0.161 ms per GiB (0.76 -> 0.83 of 8 TB/s; profiles/r03_ab_cs16_tile8192.txt).  Holding the kernel to 80 or
// 64 VGPRs for six or eight workgroups spills and is slower (0.171 / 0.188 ms).
#ifndef ADSB_KRUN_I16
#define ADSB_KRUN_I16 16
#endif
constexpr int kRunI16 = ADSB_KRUN_I16;
template <int ST> struct TileCfg {
    static constexpr int kRunT = ST == ADSB_SAMPLE_I8 ? kRun : kRunI16;
    static constexpr int kTileT = 2 * kThreads * kRunT;
    static constexpr int kMagT = kTileT + kHalo;
};
constexpr int tile_offsets(int sample_type)
{
    return sample_type == ADSB_SAMPLE_I8 ? kTile : 2 * kThreads * kRunI16;
}
constexpr int kTileMax = kTile > 2 * kThreads * kRunI16 ? kTile : 2 * kThreads * kRunI16;
// Which i8 scan kernel a context launches (adsb_create reads ADSB_SCAN from the environment; default root).  The product's
// is in adsb_kernels.hip; the other four are laboratory scans, one file each under ab/, kernels in -DADSB_AB_KERNELS=1 builds only:
//   kScanRoot: floor(sqrt(n)) per sample (v_sqrt_f32), u8 magnitudes in LDS -- the product's kernel
//   kScanNsq : the gate runs on n = I^2+Q^2 (no root per sample; exact: DESIGN.md section 4.1b), 2 bytes of LDS per
//              sample (ab/nsq.inc): the round-3 A/B kernel (fewer VALU slots, half the resident workgroups: slower)
constexpr int kScanNsq = 0, kScanRoot = 1, kScanReg = 2, kScanCode = 3, kScanSieve = 4;
//   kScanCode: the gate slides over an 8-bit LOG code of n = I^2+Q^2 (one quarter-rate v_cvt_pk_fp8_f32 per pair of samples
//              instead of a root per sample); a superset test on codes, the few uncertain survivors are decided from the
//              samples themselves (ab/code.inc): a round-4 A/B kernel (bit-exact, not faster)
//   kScanSieve: one pair of relation bits per sample (neighbouring samples compared, no root), the gate's fourteen adjacent taps as
//              shifts and ANDs of 64-bit words, the few candidates decided exactly from the raw samples kept in LDS
//              (ab/sieve.inc): the round-4 A/B kernel (bit-exact, 0.200 ms against the root scan's 0.190)
//   kScanReg : the nsq gate from registers, no LDS image (every wave a chunk of 4032 offsets; window overlap by DPP from
//              the neighbouring lane); tiles of 16128 offsets (ab/reg.inc)
constexpr int kRegTile = 4 * 2 * 63 * 32; // offsets per tile of the register scan: four waves x 4032
#ifndef ADSB_SV_SWEEPS
#define ADSB_SV_SWEEPS 8                  // 16-byte loads per lane and tile of the sieve scan (8: 16384-offset tiles, four workgroups
#endif                                    // per CU; 6: 12288, five -- measured no faster, profiles/r04_ab_sieve.txt)
constexpr int kSieveTile = ADSB_SV_SWEEPS * kThreads * 8; // offsets per tile of the sieve scan (ab/sieve.inc)
// offsets per tile of a context (the scan kind is fixed at adsb_create)
constexpr int tile_offsets_of(int sample_type, int scan)
{
    return (sample_type == ADSB_SAMPLE_I8 && scan == kScanReg) ? kRegTile
           : (sample_type == ADSB_SAMPLE_I8 && scan == kScanSieve) ? kSieveTile : tile_offsets(sample_type);
}
constexpr int kListCap = 128;   // candidate offsets staged per decode chunk
constexpr int kSparseCap = 64;  // up to this many gate survivors per tile take the cheap (rank-sort) path
constexpr int kWindow = 240;    // 16 + 112*2  (reference src/adsb.rs:98)
constexpr uint32_t kNoBase = 0xFFFFFFFFu;
// Every tile owns kQuota frame slots at a fixed place (slot = tile * kQuota + i), so the normal
// case needs no allocation at all; only a tile with more gate survivors than that draws from the
// shared pool with one returning atomic.  (One atomic per tile on a single address measured as the
// bottleneck: ~80 atomics/us per address vs 62 tiles/us.)
constexpr uint32_t kQuota = 32;
// One entry per tile, written unconditionally by the demod kernel.
struct Seg {
    uint32_t base;    // first temp slot of this tile, kNoBase if the slot store was full
    uint32_t cand;    // offsets that passed the preamble+DF17 gate (slots reserved; the scan kernel writes each survivor's offset there)
    uint32_t valid;   // of those, frames that passed CRC / single-bit repair (written by the finishing kernel)
    uint32_t decoded; // 1: `valid` is already final when the scan kernel ends (a tile without slots, counted in place)
};

// Device-resident result header (adsb_result_device).
struct Header {
    uint64_t n_out;        // frames in the final list (<= max_out)
    uint64_t total_found;  // frames that exist
    uint32_t flags;        // ADSB_FLAG_*
    uint32_t retry;        // internal: a needed tile lost its slots (slot store overflow)
    unsigned long long alloc; // pool allocator for tiles over their quota (reset by the gather kernel)
};

struct DemodArgs {
    const void *iq;            // channel 0, sample 0
    uint64_t n_samples;        // per channel
    uint64_t channel_stride;   // samples
    uint32_t tiles_per_channel;
    uint32_t tile_first;       // global tile id of blockIdx.x == 0
    uint32_t tile_count;       // workgroups in this launch
    uint32_t count_groups;     // 1: first pass of a launch (clears the header's flags); 0: re-run of known tiles
    uint32_t fused_pass_only;  // measurement (adsb_debug_fused_pass_only): magnitude + gate only, survivors counted but not decoded
    uint64_t offset_base;      // added to every frame's offset (adsb_set_stream_base: position of sample 0 in a longer stream)
    Seg *seg;
    adsb_frame *slots;         // [n_tiles_max * kQuota] fixed region, then the pool
    uint32_t pool_first;       // index of the pool's first slot
    uint32_t cap_slots;        // pool capacity
    Header *hdr;
    uint64_t *hdr_pub;         // optional caller-owned header copy (adsb_set_result_target): its flags word is cleared here
    uint32_t pool_off;         // test knob (adsb_debug_pool_limit): 1 = the shared slot pool hands out nothing
    unsigned long long *stamps; // diagnostic builds (-DADSB_TILE_STAMPS=1) only: 64 bytes of cycle counters per tile
};

// finish_order: CRC-24 / repair of the survivors + the ordered list, in one kernel (see adsb_kernels.hip)
struct FinishArgs {
    Seg *seg;
    adsb_frame *slots;
    adsb_frame *out;
    const uint32_t *out_start; // optional [n_tiles]: host-planned positions (re-run of lost tiles): no look-back, no header
    uint64_t *lb;              // exchange words (value | flag | epoch), never cleared, tagged with `epoch`: one per
    uint32_t lb_groups_at;     // workgroup from lb[0], one per 64 workgroups from lb[lb_groups_at]
    uint64_t *chan_prefix;     // optional [n_channels + 1]: frames before each channel's first tile; [n_channels] = total
    uint32_t epoch;            // launch index + 1 (30 bits)
    uint32_t tiles_per_channel;
    uint32_t n_channels;
    uint32_t max_out;
    uint32_t tile_first, tile_count;
    Header *hdr;
    uint64_t *hdr_pub;         // optional caller-owned copy of {n_out, total_found, flags} (4 x u64)
    uint32_t stall_blk;        // test knob (adsb_debug_finish_stall): this workgroup withholds its exchange word; 0xFFFFFFFF: none
};

// demod_small: the one-dispatch path for buffers of at most kFinishTilesPerWg tiles
struct SmallArgs {
    uint32_t *done;      // device word, zero between launches: workgroups that have finished their tile
    uint64_t *seq_host;  // host-visible (pinned) word the last workgroup writes `seq` to when header and list are complete
    uint64_t seq;
};

// mag_mode: how v_cvt_pk_u8_f32 rounds on this device (decided once per ctx by probe_cvt):
//   0: truncates as is; 1: truncates once MODE.fp_round(f32) is set to round-toward-zero;
//   2: rounds to nearest regardless -> subtract 0.5 first.
hipError_t probe_cvt(hipStream_t s, uint32_t *dev_scratch4, uint32_t host_out[4]);
// the code scan's arithmetic on every n = 0 .. 32768: out[n] = c(n) | byte1(S(c(n) << 8)) << 8 (device buffer of 32769 u16)
hipError_t launch_code_probe(hipStream_t s, uint16_t *dev_out32769);

// e0/e1: optional events recorded at the start / end of the dispatch itself (nullptr: none)
// scan: kScanNsq / kScanRoot (i8 only; CS16 has one kernel)
hipError_t launch_demod(hipStream_t s, int sample_type, int mag_mode, int scan, const DemodArgs &a,
                        hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr);
// second kernel of a launch (finish_order): CRC-24 + single-bit repair of the survivors the scan kernel sliced into
// their slots, and the ordered frame list
hipError_t launch_finish(hipStream_t s, const FinishArgs &a, hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr);
// finish_order's constants (adsb_debug_finish_geometry; each optional): tiles per workgroup, workgroups per second-level
// sum, the largest grid that exchanges in one level, second-level sums a wave reads per round
void finish_geometry(uint32_t *tiles_per_workgroup, uint32_t *fan, uint32_t *flat, uint32_t *sums_per_round);
// the header of an empty list (no tiles, or a measurement launch without the finishing kernel)
hipError_t launch_empty_result(hipStream_t s, Header *hdr, uint64_t *hdr_pub, uint64_t *chan_prefix, uint32_t n_channels,
                               hipEvent_t e0 = nullptr, hipEvent_t e1 = nullptr);
constexpr int kFinishTilesPerWg = 32;
// scan + finish in one dispatch for 1..kFinishTilesPerWg tiles; the list goes to f.out / f.hdr_pub (host-visible memory)
hipError_t launch_small(hipStream_t s, int sample_type, int mag_mode, int scan, const DemodArgs &p, const FinishArgs &f,
                        const SmallArgs &sm);

bool ab_kernels_built();  // -DADSB_AB_KERNELS=1: the A/B scan kernels (nsq, reg, code, sieve) are in this library
bool tile_stamps_built(); // -DADSB_TILE_STAMPS=1 diagnostic build: DemodArgs::stamps holds 64 bytes per tile

// field decode of an ordered frame list (count read from hdr->n_out on the device)
hipError_t launch_decode_fields(hipStream_t s, const adsb_frame *frames, const Header *hdr, uint32_t cap,
                                adsb_packet_fields *out); // hdr == nullptr: exactly cap frames

// per-frame power statistics of an ordered frame list (adsb_levels.hip): one wavefront per frame reads the 240 samples
// the frame was decoded from
struct LevelsArgs {
    const void *iq;              // channel 0, sample 0 (device-visible; aligned to one sample)
    uint64_t n_samples;          // per channel
    uint64_t channel_stride;     // samples between channel starts
    uint64_t offset_base;        // frame i sits at sample frames[i].offset - offset_base of its channel
    const adsb_frame *frames;
    const Header *hdr;           // count = min(hdr->n_out, cap), read on the device; nullptr: exactly cap frames
    uint32_t cap;
    uint32_t n_channels;         // 1: every frame is channel 0's and chan_prefix is not read
    const uint64_t *chan_prefix; // [n_channels + 1]: frames of the list before each channel's first
    adsb_frame_level *out;       // [cap]
};
// blocks: the grid (4 waves per block, frames in a grid-stride loop); sized from the device by the caller
hipError_t launch_frame_levels(hipStream_t s, int sample_type, const LevelsArgs &a, uint32_t blocks);

// level records by frame length, of a caller's list over many channels (adsb_levels.hip, frame_levels_modes_kernel;
// adsb_levels.h has the per-frame text)
struct LevelsModesArgs {
    const void *iq;              // channel 0, sample 0 (device-visible; aligned to one sample)
    uint64_t n_samples;          // per channel
    uint64_t channel_stride;     // samples between channel starts
    uint64_t offset_base;        // frame i sits at sample frames[i].offset - offset_base of its channel
    const adsb_frame *frames;    // [n]
    uint32_t n;
    uint32_t n_channels;         // 1: every frame is channel 0's and prefix is not read
    const uint64_t *prefix;      // [n_channels + 1]: frames of the list before each channel's first; last = n
    adsb_frame_level *out;       // [n]
};
hipError_t launch_frame_levels_modes(hipStream_t s, int sample_type, const LevelsModesArgs &a, uint32_t blocks);

// an ordered frame list as one stream of Beast binary or AVR text (adsb_wire.hip): three dispatches, see there
constexpr uint32_t kWireBlockFrames = 256; // frames (= threads) per workgroup of the lengths and write kernels
constexpr uint32_t kWireScanThreads = 256; // threads of the one workgroup that scans the workgroups' totals
constexpr uint32_t wire_blocks(uint64_t cap) { return (uint32_t)((cap + kWireBlockFrames - 1) / kWireBlockFrames); }
struct WireArgs {
    const adsb_frame *frames;
    const adsb_frame_level *levels; // [cap], or null: signal byte 0
    const Header *hdr;           // count = min(hdr->n_out, cap), read on the device; nullptr: exactly cap frames
    uint32_t cap;                // 44 x cap < 2^32
    uint32_t format;             // ADSB_WIRE_*
    int sample_type;             // the full scale of the signal byte
    uint64_t tick_bias;
    uint8_t *out;                // [44 x cap], dword-aligned
    uint32_t *ends;              // [cap]
    uint32_t *block;             // [wire_blocks(cap)]: each workgroup's total, then where its span starts
    uint64_t *wire_hdr;          // {bytes in the stream, frames in it}
};
hipError_t launch_wire(hipStream_t s, const WireArgs &a);

// byte streams of Beast binary or AVR text back into an ordered frame list (adsb_wire_in.hip): six dispatches, see there
constexpr uint32_t kWireInBlockBytes = 4096; // bytes of the stream per workgroup span
constexpr uint32_t kWireInThreads = 256;     // threads per span: 16 bytes each
constexpr uint32_t kWireInScanThreads = 256; // threads of the one workgroup that scans the spans' words
static_assert(kWireInThreads * 16 == kWireInBlockBytes, "16 bytes per thread");
struct WireInTally;                          // adsb_wire_in.h
struct WireInArgs {
    const uint32_t *words;       // the dword that holds bytes[0]: stream byte g is byte g + lead from here
    uint32_t lead;               // 0..3
    uint32_t n_bytes;
    uint32_t n_streams;          // 1..256
    const uint32_t *ends;        // [n_streams] ascending exclusive ends, the last = n_bytes
    uint32_t format, filter;     // ADSB_WIRE_*, ADSB_WIRE_IN_*
    uint64_t tick_bias;
    int sample_type;             // the full scale of the level records
    uint32_t cap;                // frames kept
    uint32_t n_spans;            // ceil((lead + n_bytes) / kWireInBlockBytes)
    // scratch
    uint32_t *last;              // [n_spans] 1 + the place in its span of the span's last byte that is not 0x1A; 0: none
    uint64_t *carry;             // [n_spans] 1 + (lead + the position) of the last such byte in front of the span; 0: none
    WireInTally *tally;          // [n_spans] the span's counters; `kept` becomes the list index of its first frame
    uint32_t *inc, *tail;        // [n_streams] 1 + the incomplete mark's position (0: none); consumed without one
    // results
    adsb_frame *frames;          // [cap]
    adsb_wire_rx *rx;            // [cap]
    adsb_frame_level *levels;    // [cap] or null
    uint64_t *counts, *consumed; // [n_streams]
    adsb_wire_in_header *hdr;
};
constexpr uint32_t wire_in_spans(uint64_t lead_plus_bytes) { return (uint32_t)((lead_plus_bytes + kWireInBlockBytes - 1) / kWireInBlockBytes); }
hipError_t launch_wire_in(hipStream_t s, const WireInArgs &a);

// receptions of one transmission across receivers (adsb_correlate.hip): the dispatch sequence is described there
constexpr uint32_t kCorrBlock = 256; // receptions (= threads) per workgroup of the key and write kernels
struct CorrAgg;                      // adsb_correlate.h
struct CorrArgs {
    const adsb_frame *frames;        // [n], adsb_fetch's layout
    const adsb_frame_level *levels;  // [n] or null
    uint32_t n, n_receivers, window;
    const uint64_t *prefix;          // [n_receivers + 1]: list index of each receiver's first frame; last = n
    const uint64_t *base;            // [n_receivers] or null: all 0
    // scratch, [n] each
    uint64_t *t, *lo, *hi, *head_t;  // per list index: T and the key words; per sorted position: the head's T, sorted
    uint32_t *rx, *ord, *pos, *midx; // receiver per list index; list index per group-order position; group-order
                                     // position per output position; heads up to and including an output position
    CorrAgg *scan;                   // per group-order position: the aggregate of its group up to it
    void *temp;
    size_t temp_bytes;               // >= corr_temp_bytes(n)
    // results
    adsb_message *msgs;              // [n]
    adsb_frame *frames_out;          // [n]
    adsb_reception *recs;            // [n]
    uint64_t *hdr;                   // {n_messages, n_receptions}
};
size_t corr_temp_bytes(size_t n);
hipError_t launch_correlate(hipStream_t s, const CorrArgs &a);

// every frame's address and surveillance fields (adsb_modes.hip: the dispatch sequence is described there)
constexpr uint32_t kModesBlock = 256; // frames (= threads) per workgroup of the stage's kernels
constexpr uint32_t modes_blocks(uint64_t n) { return (uint32_t)((n + kModesBlock - 1) / kModesBlock); }
struct ModesArgs {
    const adsb_frame *frames;        // [n], adsb_fetch's layout
    const uint32_t *known_in;        // [n_known_in] ascending, unique, < 2^24
    const uint64_t *prefix;          // [n_receivers + 1] frames in front of each receiver, last = n; null: no counts
    uint32_t n, n_known_in, n_receivers;
    // scratch; m = n_known_in + n entries
    uint32_t *key, *val;             // [m] known_in's (address, 0), then per frame (address or 2^24, 1 + index)
    uint32_t *key_s, *val_s;         // [m] the same in stable address order
    uint32_t *hidx;                  // [m] heads of address runs up to and with each sorted entry
    uint32_t *first;                 // [m] per known_out entry: 0 (of known_in) or 1 + the index of its first SELF frame
    uint32_t *sidx;                  // [n] squitters up to and with each frame
    uint32_t *tally;                 // [5 x modes_blocks(n)] the kinds of each workgroup's frames
    void *temp;
    size_t temp_bytes;               // >= modes_temp_bytes(capacity)
    // results
    adsb_modes_rec *recs;            // [n]
    uint32_t *known_out;             // [m]
    adsb_frame *squitters;           // [n]
    uint64_t *sq_counts;             // [256]
    adsb_modes_header *hdr;
};
size_t modes_temp_bytes(size_t m);
hipError_t launch_modes(hipStream_t s, const ModesArgs &a);

// the Comm-B register of every DF20/21 frame and its values (adsb_commb.hip; adsb_commb.h has the text of one frame)
constexpr uint32_t kCommbBlock = 256; // frames (= threads) per workgroup of commb_frames
constexpr uint32_t kCommbTallyWords = 12; // per workgroup: the five states, then the ONE records of the seven registers
constexpr uint32_t commb_blocks(uint64_t n) { return (uint32_t)((n + kCommbBlock - 1) / kCommbBlock); }
struct CommbArgs {
    const adsb_frame *frames; // [n], adsb_fetch's layout
    uint32_t n;
    uint32_t *tally;          // [kCommbTallyWords x commb_blocks(n)]
    // results
    adsb_commb_rec *recs;     // [n], 16-byte aligned
    adsb_commb_header *hdr;
};
hipError_t launch_commb(hipStream_t s, const CommbArgs &a);

// the extended squitter status of every DF17/18 frame (adsb_es.hip; adsb_es.h has the text of one frame)
constexpr uint32_t kEsBlock = 256; // frames (= threads) per workgroup of es_frames
constexpr uint32_t kEsTallyWords = 14; // per workgroup: the ten states, then the OPERATIONAL records of version 0, 1, 2, 3-7
constexpr uint32_t es_blocks(uint64_t n) { return (uint32_t)((n + kEsBlock - 1) / kEsBlock); }
struct EsArgs {
    const adsb_frame *frames; // [n], adsb_fetch's layout
    uint32_t n;
    uint32_t *tally;          // [kEsTallyWords x es_blocks(n)]
    // results
    adsb_es_rec *recs;        // [n], 16-byte aligned
    adsb_es_header *hdr;
};
hipError_t launch_es(hipStream_t s, const EsArgs &a);

// Mode S replies from samples (adsb_replies.hip: the dispatch sequence is described there; adsb_replies.h has the text of
// one offset and of one frame)
constexpr uint32_t kRepliesGroupTiles = 4096; // tiles per workgroup of the two folding kernels
constexpr uint32_t replies_groups(uint64_t n_tiles) { return (uint32_t)((n_tiles + kRepliesGroupTiles - 1) / kRepliesGroupTiles); }
struct RepliesArgs {
    const void *iq;              // channel 0, sample 0; 16-byte aligned
    uint64_t n_samples;          // per channel
    uint64_t channel_stride;     // samples, a multiple of 8
    uint64_t offset_base;        // added to every frame's offset
    uint32_t n_channels, tiles_per_channel, n_tiles;
    uint32_t flags;              // ADSB_REPLIES_*
    const uint32_t *known;       // [n_known] ascending, distinct
    uint32_t n_known;
    uint32_t cap;                // frames kept
    // scratch
    uint32_t *tile;              // [7][n_tiles]: per tile the frames kept, then the six counts of adsb_replies.h
    uint32_t *bitmap;            // [n_tiles][256]: a tile's kept offsets, one word per thread's run; written only by a
                                 // tile that keeps a frame
    uint32_t *group;             // [7][replies_groups(n_tiles)]: the same seven summed over each group of tiles
    uint64_t *prefix;            // [n_tiles + 1]: frames kept in front of each tile; last = all
    // results
    adsb_frame *frames;          // [cap]
    uint64_t *counts;            // [n_channels]
    adsb_replies_header *hdr;
};
hipError_t launch_replies(hipStream_t s, int sample_type, const RepliesArgs &a);
// two per-channel-ordered lists as one (merge_lists, adsb_replies.hip)
struct MergeArgs {
    const adsb_frame *a, *b;     // [na], [nb]
    const uint64_t *prefix_a, *prefix_b; // [n_channels + 1] each
    uint32_t n_channels, na, nb;
    adsb_frame *out;             // [na + nb]
    uint32_t *src;               // [na + nb] or null
};
hipError_t launch_merge_lists(hipStream_t s, const MergeArgs &a);

// transmitter positions from correlated receptions (adsb_mlat.hip; adsb_mlat.h has the solver's text)
constexpr uint32_t kMlatBlock = 256;                          // threads per workgroup of mlat_solve
constexpr uint32_t kMlatPerBlock = kMlatBlock / kMlatLanes;   // messages per workgroup: 16 lanes each
struct MlatArgs {
    const adsb_message *msgs;        // [n_msgs]
    const adsb_reception *recs;      // [n_recs]
    const adsb_wire_rx *rx;          // [n_rx] or null (TIME_RECEPTION)
    const uint64_t *counts_dev;      // null, or {n_msgs, n_recs} in device memory (a correlate header): the counts below
                                     // are then upper bounds that size the grid, and these the lists' lengths
    uint32_t n_msgs, n_recs, n_rx, n_receivers;
    const MlatStation *stations;     // [n_receivers]
    MlatParams p;
    void *temp;
    size_t temp_bytes;               // >= mlat_temp_bytes(n_msgs)
    // results
    adsb_mlat_fix *fixes;            // [n_msgs]
    adsb_mlat_header *hdr;
};
size_t mlat_temp_bytes(size_t n_msgs);
hipError_t launch_mlat(hipStream_t s, const MlatArgs &a);

// receiver clocks from position messages (adsb_clock.hip; adsb_clock.h has the shared text)
constexpr uint32_t kClockBlock = 256;                           // threads per workgroup of every clock kernel
constexpr uint32_t kClockPerBlock = kClockBlock / kClockLanes;  // messages per workgroup of the rows and apply kernels
struct ClockArgs {
    const adsb_message *msgs;        // [n_msgs]
    const adsb_reception *recs;      // [n_recs]
    const adsb_wire_rx *rx;          // [n_rx] or null (TIME_RECEPTION)
    const uint64_t *counts_dev;      // as MlatArgs'
    uint32_t n_msgs, n_recs, n_rx, n_receivers;
    const ClockStation *stations;    // [n_receivers]
    ClockParams p;
    void *temp;
    size_t temp_bytes;               // >= clock_temp_bytes(n_recs)
    // scratch
    double *tau, *yp;                // [n_recs] each: the rows, slot for slot
    uint32_t *key, *key_sorted, *slot_sorted; // [n_recs] each
    uint8_t *msg_flags;              // [n_msgs]
    ClockPair *pairs, *pairs_first;  // [256 x 256] each: the sums of the last pass, and of the first
    double *normal;                  // [kClockMaxUnknowns x kClockMaxUnknowns]
    ClockSol *sol;                   // [256]
    // results
    adsb_clock *clocks;              // [n_receivers]
    adsb_clock_header *hdr;
    adsb_reception *corrected;       // [n_recs]
};
size_t clock_temp_bytes(size_t n_recs);
hipError_t launch_clock_sync(hipStream_t s, const ClockArgs &a);
hipError_t launch_clock_apply(hipStream_t s, const ClockArgs &a);

// tracker + CPR position decode over an ordered frame list (adsb_track.hip)
// One aircraft of a persistent table (adsb_track_table_*): the public record plus the last even and the last odd
// position message (aircraft.rs:28-31) that a later update's first position message of the other format pairs with.
struct TrackRecord {
    adsb_aircraft_record a;      // n_frames: frames since create / reset
    double t_even, t_odd;        // time of the last even / odd position message
    uint32_t even_lat, even_lon, odd_lat, odd_lon;
    uint32_t have;               // bit 0: an even position message was seen, bit 1: an odd one
    uint32_t pad;
    double last_heard;           // time of the last frame of any kind (adsb_track_*_expire evicts on it)
    adsb_velocity vel;           // the last airborne-velocity message (TC 19, ST 1-4); subtype 0 = none yet
};
static_assert(sizeof(TrackRecord) == 128, "TrackRecord: one cache line; the header's memory figures assume 128 bytes");
constexpr uint32_t kTrackUntracked = 0xFFFFFFFFu; // slot of an aircraft the full table turned away
// The three forms of the tracker: one launch's list from an empty map (adsb_track_device), a persistent table
// (adsb_track_table_*), a bank of persistent tables, one per receiver (adsb_track_bank_*).  The one thing that tells them
// apart, in TrackArgs / ExpireArgs and as the kernels' template parameter.
enum class TrackKind : uint32_t { kLaunch, kTable, kBank };
// The device view of a table or bank.  A table is the n_receivers == 1 case of the common part and finds an aircraft
// through a direct ICAO index; a bank sorts by receiver << 24 | icao and probes an open-addressing hash of that key
// (a direct index per receiver would cost 64 MiB each), with per-frame scan words of its own.
struct TrackStoreDev {
    // common
    TrackRecord *rec;            // [n_receivers x max_aircraft]: receiver r's records at [r x max_aircraft, ...)
    uint32_t max_aircraft;       // per receiver
    uint32_t n_receivers;        // a table: 1
    uint32_t *size;              // [n_receivers] records in use
    uint32_t *flags;             // [n_receivers] ADSB_TRACK_TABLE_FULL
    uint32_t *size_next;         // [n_receivers] staging: the admission kernel's new sizes, moved to size by the pairs
                                 // kernel; expire stages the old sizes here
    uint32_t *slot;              // [n] scratch: record slot + 1 of each sorted frame's aircraft (kTrackUntracked)
    adsb_aircraft_level *lvl;    // [n_receivers x max_aircraft] beside rec, or null: no levels reserve (then admission
                                 // and expire touch nothing more than they did)
    adsb_fix *fix;               // [n_receivers x max_aircraft] beside rec, or null: no fixes reserve (likewise)
    const adsb_site *site;       // [n_receivers] with fix: the site receiver r's frames decode against
    adsb_aircraft_mlat *mlat;    // [n_receivers x max_aircraft] beside rec, or null: no mlat reserve (likewise; tables only)
    adsb_aircraft_modes *modes;  // [max_aircraft] beside rec, or null: no modes reserve (likewise; tables only)
    // table only
    uint32_t *index;             // [1 << 24]: ICAO -> record slot + 1, 0 = absent
    // bank only
    unsigned long long *hash;    // [hash_mask + 1]: (record slot + 1) << 32 | key, 0 = empty (insert by atomicCAS)
    uint64_t hash_mask;          // capacity - 1, capacity a power of two >= 2 x n_receivers x max_aircraft
    uint32_t key_bits;           // 24 + ceil(log2 n_receivers)
    uint32_t *prefix;            // [n_receivers + 1]: frames of the list before each receiver's first (last = n); also
                                 // where each receiver's first frame sits in sorted order
    const uint64_t *sample_base; // [n_receivers]: frame time = (sample_base[r] + offset) x seconds_per_sample
    const uint64_t *src_prefix;  // [n_src + 1] (device): the receiver split as given (host counts' prefix, or the
    uint32_t n_src;              // launch's chan_prefix); clipped to n into `prefix`, receivers >= n_src get nothing
    unsigned long long *mark;    // [n] per sorted frame: segment head << 32 | head of a key the hash does not hold
    unsigned long long *excl;    // [n] exclusive scan of mark
    uint32_t *seg_slot;          // [n] per segment (hi of the scan): record slot + 1 (kTrackUntracked)
    // table only, last so that no other member moves
    adsb_aircraft_commb *commb;  // [max_aircraft] beside rec, or null: no commb reserve (likewise; tables only)
    adsb_aircraft_es *es;        // [max_aircraft] beside rec, or null: no es reserve (likewise; tables only)
    adsb_aircraft_filter *filter; // [max_aircraft] beside rec, or null: no filter reserve (likewise; tables only)
};
// Per-frame summaries and the changed list of a table / bank update (adsb_track_*_summaries_reserve): all of it
// allocated by the reserve.  One segmented inclusive max-scan over the sorted list gives every frame the sorted
// position + 1 (0 = none in its segment so far) of its segment's head and of the last identification message,
// position message and frame with a new position at or before it; cnt is a plain running sum of the segment heads
// the table tracks, which ranks the changed list.
struct TrackSumTuple {
    uint32_t head, id, pos, fix, cnt;
};
struct TrackSumDev {
    TrackSumTuple *scan;         // [max_frames]: the scan's output, sorted order
    adsb_aircraft_record *out;   // [max_frames]: one summary per frame of the last update, list order
    uint32_t *changed;           // [max_frames]: record slot of every tracked segment, sorted order (= ascending ICAO)
    uint32_t *n_changed;         // device word: how many of them
    void *temp;                  // the scan's scratch
    size_t temp_bytes;
};
// Per-aircraft signal levels of a table / bank update (adsb_track_*_levels_reserve): all of it allocated by the reserve.
// One segmented inclusive scan over the sorted list sums, per aircraft, what its COUNTED frames carry (tracked, and the
// frame's level record valid); every component combines by saturating add, max, or "the later sorted position", so the
// result does not depend on how rocPRIM groups the operands.  newest = sorted position + 1 of the last counted frame,
// 0 = none: last_* are read from that frame by the tail kernel, not carried.
struct TrackLvlTuple {
    uint64_t signal, noise, max_signal;
    uint32_t n, peak, weak, newest;
    uint32_t head;               // the operand holds a segment head
    uint32_t pad;
};
static_assert(sizeof(TrackLvlTuple) == 48, "TrackLvlTuple: the header's memory figures assume 48 bytes");
struct TrackLvlDev {
    TrackLvlTuple *scan;         // [max_frames]: the scan's output, sorted order
    void *temp;                  // the scan's scratch
    size_t temp_bytes;
};
// Positions from single messages (adsb_track_*_fixes_reserve; adsb_fix.h has the decode): all of it allocated by the
// reserve.  One thread per sorted frame decodes into out / rem at the frame's list index; one segmented inclusive scan
// over the sorted list carries, per aircraft, the sorted position + 1 of the later ACCEPTED position message (0 = none)
// and saturating counts of accepted and rejected ones; one thread per segment tail merges into store->fix.
struct TrackFixTuple {
    uint32_t head;               // the operand holds a segment head
    uint32_t newest, n_ok, n_rej;
};
struct FixRem;                   // adsb_fix.h: 16 bytes per frame
struct TrackFixDev {
    adsb_frame_fix *out;         // [max_frames]: one per frame of the last update, list order
    FixRem *rem;                 // [max_frames]: the rest of what a fix takes from its frame, list order
    TrackFixTuple *scan;         // [max_frames]: the scan's output, sorted order
    void *temp;                  // the scan's scratch
    size_t temp_bytes;
};
// Multilaterated positions per aircraft (adsb_track_table_mlat_reserve; adsb_track_mlat.h has the per-frame text): all of
// it allocated by the reserve.  One thread per sorted frame writes out[] at the frame's list index and the scan's operand
// at its sorted position; one segmented inclusive scan carries, per aircraft, the sorted position + 1 of the later frame
// with a VALID fix and of the later CHECKED frame (0 = none), the greatest disagreement and four saturating counts; one
// thread per segment tail merges into store->mlat.  Integers and one float max: the scan's shape cannot show.
struct TrackMlatTuple {
    uint32_t head;               // the operand holds a segment head
    uint32_t newest_valid, newest_checked;
    float max_m;                 // >= 0, never NaN
    uint32_t n_attempted, n_valid, n_checked, n_disagree;
};
static_assert(sizeof(TrackMlatTuple) == 32, "TrackMlatTuple: the header's memory figures assume 32 bytes");
struct TrackMlatDev {
    adsb_frame_mlat *out;        // [max_frames]: one per frame of the last update_mlat, list order
    TrackMlatTuple *in;          // [max_frames]: the scan's operands, sorted order
    TrackMlatTuple *scan;        // [max_frames]: the scan's output, sorted order
    void *temp;                  // the scan's scratch
    size_t temp_bytes;
    double max_disagreement_m;   // the reserve's limit
};
// Filtered mlat track per aircraft (adsb_track_table_filter_reserve; adsb_track_filter.h has the operand's and the
// step's text): all of it allocated by the reserve.  One thread per sorted frame writes the operand at its sorted
// position; one thread per segment head walks its segment's operands through the record at store->filter and writes
// out[] at each usable frame's list index.  No scan, no scratch.
struct TrackFilterDev {
    adsb_filter_operand *op;     // [max_frames]: the last update's operands, sorted order
    adsb_frame_filter *out;      // [max_frames]: one per frame of the last update given fixes, list order
    adsb_track_filter_cfg cfg;   // the reserve's, every default filled in
};
// Mode S replies per aircraft (adsb_track_table_modes_reserve; adsb_track_modes.h has the per-frame text and the
// combine): all of it allocated by the reserve.  One thread per sorted frame writes the scan's operand at its sorted
// position; one segmented inclusive scan carries, per aircraft, the sorted position + 1 of the later counted frame that
// writes each field (0 = none), four saturating counts and the squitter bit; one thread per segment tail reads the
// winning frames' records and merges into store->modes.  Integers only: the scan's shape cannot show.
struct TrackModesTuple {
    uint32_t head;               // the operand holds a segment head
    uint32_t squitter;           // a counted DF17/18 frame
    uint32_t alt, squawk, callsign, status, ground, any; // newest counted frame of each sort
    uint32_t n_replies, n_allcall, n_surveillance, n_airair;
};
static_assert(sizeof(TrackModesTuple) == 48, "TrackModesTuple: the header's memory figures assume 48 bytes");
// Comm-B registers per aircraft (adsb_track_table_commb_reserve; adsb_track_commb.h has the rule, the per-frame text
// and the combine): all of it allocated by the reserve.  A segmented scan of TrackCommbRefTuple gives every sorted frame
// its aircraft's newest velocity frame up to it (the frame kernel reads its predecessor's: the exclusive scan); one
// thread per sorted frame settles, writes the per-frame output at the list index and the second scan's operand at the
// sorted position; one segmented inclusive scan; one thread per segment tail merges into store->commb.  Integers only.
struct TrackCommbRefTuple {
    uint32_t head;               // the operand holds a segment head
    uint32_t vel;                // sorted position + 1 of the newest velocity frame, 0 = none
};
struct TrackCommbTuple {
    uint32_t head;
    uint32_t newest[5];          // sorted position + 1 of the newest counted frame of sort 4,0 / 5,0 / 6,0 / 1,7 / 3,0
    uint32_t n_commb, n_settled, n_ambiguous, n_none;
};
static_assert(sizeof(TrackCommbTuple) == 40 && sizeof(TrackCommbRefTuple) == 8, "the header's memory figures");
struct TrackCommbDev {
    TrackCommbRefTuple *ref;     // [max_frames]: the first scan's output, sorted order
    adsb_commb_rec *out;         // [max_frames]: the per-frame output of the last update_commb, list order
    TrackCommbTuple *in;         // [max_frames]: the second scan's operands, sorted order
    TrackCommbTuple *scan;       // [max_frames]: its output, sorted order
    void *temp;                  // both scans' scratch
    size_t temp_bytes;
    adsb_commb_settle_cfg cfg;   // the reserve's
};
// Extended squitter status per aircraft (adsb_track_table_es_reserve; adsb_track_es.h has the rule, the per-frame text
// and the combine): all of it allocated by the reserve.  A segmented scan of TrackEsRefTuple gives every sorted frame
// its aircraft's newest frames with a version, a supplement A and a supplement C up to it (the frame kernel reads its
// predecessor's: the exclusive scan); one thread per sorted frame resolves, writes the per-frame output at the list
// index and the second scan's operand at the sorted position; one segmented inclusive scan; one thread per segment
// tail merges into store->es.  Integers and one f64 subtraction for an age.
struct TrackEsRefTuple {
    uint32_t head;               // the operand holds a segment head
    uint32_t version, a, c;      // sorted position + 1 of the newest frame with HAS_VERSION / HAS_NIC_A / HAS_NIC_C, 0 = none
};
struct TrackEsTuple {
    uint32_t head;
    uint32_t newest[11];         // sorted position + 1 of the newest counted frame that writes group g (adsb_track_es.h)
    uint32_t n_es, n_position;
};
static_assert(sizeof(TrackEsTuple) == 56 && sizeof(TrackEsRefTuple) == 16, "the header's memory figures");
struct TrackEsDev {
    TrackEsRefTuple *ref;        // [max_frames]: the first scan's output, sorted order
    adsb_frame_integrity *out;   // [max_frames]: the per-frame output of the last update_es, list order
    TrackEsTuple *in;            // [max_frames]: the second scan's operands, sorted order
    TrackEsTuple *scan;          // [max_frames]: its output, sorted order
    void *temp;                  // both scans' scratch
    size_t temp_bytes;
    double max_age_s;            // the reserve's
};
struct TrackModesDev {
    TrackModesTuple *in;         // [max_frames]: the scan's operands, sorted order
    TrackModesTuple *scan;       // [max_frames]: the scan's output, sorted order
    void *temp;                  // the 25-bit sort's, the admission scan's and this scan's scratch
    size_t temp_bytes;
};
struct TrackArgs {
    const adsb_frame *frames;
    const adsb_packet_fields *fields;
    uint32_t n;                  // frames in the list (host value)
    double seconds_per_sample;
    uint64_t sample_base;        // frame time = (sample_base + offset) x seconds_per_sample
    uint32_t *keys, *vals, *skeys, *svals; // [n] each (keys/vals are reused as tail flags / positions)
    void *temp;
    size_t temp_bytes;
    adsb_track_point *points;    // [n], frame order
    adsb_aircraft_record *aircraft; // [max_aircraft], ascending ICAO (per-launch form only)
    uint32_t max_aircraft;
    uint64_t *n_aircraft;        // device word (per-launch form only)
    TrackKind kind;              // kLaunch: start from an empty map and summarise into `aircraft` (adsb_track_device);
                                 // kTable: pair with and merge into the persistent table (adsb_track_table_update);
                                 // kBank: the list holds several receivers' frames (adsb_track_bank_update)
    const TrackStoreDev *store;  // the table / bank (kLaunch: unused)
    const TrackSumDev *sum;      // non-null (table / bank only): also the per-frame summaries and the changed list
    const adsb_frame_level *levels; // [n] (device), list order: with lvl non-null (and store->lvl), merged into the
    const TrackLvlDev *lvl;      // per-aircraft level records; null: the level records stay as they are
    const TrackFixDev *fix;      // non-null (with store->fix and store->site): also the per-frame fixes and their merge
    const adsb_mlat_fix *mlat_fixes; // [n] (device), list order: with mlat non-null (and store->mlat), merged into the
    const TrackMlatDev *mlat;    // per-aircraft mlat records; null: the mlat records stay as they are
    const TrackFilterDev *filter; // non-null (with mlat and store->filter): also the filter behind the mlat merge
    const adsb_commb_rec *commb_recs; // [n] (device), list order: with commb non-null (and modes, store->commb): the
    const TrackCommbDev *commb;       // commb step after the modes merge (update_commb); null: the commb records stay
    const adsb_es_rec *es_recs;       // [n] (device), list order: with es non-null (and store->es): the es step beside
    const TrackEsDev *es;             // the levels / fix merges (update_es); null: the es records stay as they are
    const adsb_modes_rec *modes_recs; // [n] (device), list order: with modes non-null (and store->modes; tables only)
    const TrackModesDev *modes;  // the list is keyed by the records' addresses (update_modes); null: by bytes[1..3]
    adsb_packet_fields *modes_fields; // = fields, writable: update_modes makes every other DF a frame of kind "other"
};
// expire (adsb_track_table_expire / adsb_track_bank_expire): a record survives unless last_heard < before[receiver]
constexpr uint32_t kMaxReceivers = 256;
struct ExpireCut {
    double before[kMaxReceivers]; // [0] for a table
};
struct ExpireArgs {
    TrackKind kind;              // kTable or kBank
    const TrackStoreDev *store;
    ExpireCut cut;
    uint32_t *keep, *rank;       // [n_rec] each, n_rec = max_aircraft (x n_receivers)
    void *temp;
    size_t temp_bytes;
};
size_t track_expire_temp_bytes(size_t n_rec);
hipError_t launch_track_expire(hipStream_t s, const ExpireArgs &a);
size_t track_sort_temp_bytes(size_t n);
size_t track_bank_temp_bytes(size_t n); // the bank's sort (32 bits) and 64-bit scan
hipError_t launch_track(hipStream_t s, const TrackArgs &a);
size_t track_summaries_temp_bytes(size_t n);
size_t track_levels_temp_bytes(size_t n);
// every level record of [0, places) empty: zeros, last_time NaN (the levels reserve)
hipError_t launch_track_levels_clear(hipStream_t s, adsb_aircraft_level *lvl, size_t places);
size_t track_fixes_temp_bytes(size_t n);
// every fix of [0, places) empty: zeros, time NaN (the fixes reserve, and reset)
hipError_t launch_track_fixes_clear(hipStream_t s, adsb_fix *fix, size_t places);
size_t track_mlat_temp_bytes(size_t n);
// every mlat record of [0, places) empty: zeros, time NaN (the mlat reserve, and reset)
hipError_t launch_track_mlat_clear(hipStream_t s, adsb_aircraft_mlat *mlat, size_t places);
// every filter record of [0, places) empty: zeros, time NaN (the filter reserve, and reset)
hipError_t launch_track_filter_clear(hipStream_t s, adsb_aircraft_filter *filter, size_t places);
size_t track_modes_temp_bytes(size_t n); // the 25-bit sort, the admission scan and the modes scan
// every modes record of [0, places) empty: zeros, the three times NaN (the modes reserve, and reset)
hipError_t launch_track_modes_clear(hipStream_t s, adsb_aircraft_modes *modes, size_t places);
size_t track_commb_temp_bytes(size_t n); // the two commb scans
// every commb record of [0, places) empty: zeros, every time NaN (the commb reserve, and reset)
hipError_t launch_track_commb_clear(hipStream_t s, adsb_aircraft_commb *commb, size_t places);
size_t track_es_temp_bytes(size_t n); // the two es scans
// every es record of [0, places) empty: zeros, every time NaN (the es reserve, and reset)
hipError_t launch_track_es_clear(hipStream_t s, adsb_aircraft_es *es, size_t places);
// out[k] = rec[sum.changed[k]] for k < min(*sum.n_changed, max_n): the changed list's records, gathered on the device
hipError_t launch_track_changed(hipStream_t s, const TrackRecord *rec, const TrackSumDev &sum, uint32_t max_n,
                                TrackRecord *out);

// the fused view of a bank (adsb_track_bank_fuse): every receiver's contributing records sorted by ICAO then receiver
// and reduced to one adsb_fused_aircraft per ICAO; reads the bank only
static_assert(sizeof(adsb_fused_aircraft) == 128 && offsetof(adsb_fused_aircraft, velocity_time) == 80 &&
                  offsetof(adsb_fused_aircraft, reserved) == 80 + sizeof(adsb_velocity) &&
                  offsetof(adsb_fused_aircraft, velocity_reserved) == 80 + offsetof(adsb_velocity, reserved),
              "adsb_fused_aircraft: one cache line, an adsb_velocity bit for bit at offset 80");
static_assert(sizeof(adsb_aircraft_level) == 64 && sizeof(adsb_fused_level) == 96 &&
                  offsetof(adsb_fused_level, strongest_last_time) == offsetof(adsb_aircraft_level, last_time) &&
                  offsetof(adsb_fused_level, strongest_reserved) == offsetof(adsb_aircraft_level, reserved) &&
                  offsetof(adsb_fused_level, signal_total) == 64,
              "adsb_fused_level: an adsb_aircraft_level bit for bit at offset 0, then the sums");
constexpr uint32_t kFuseWideReceivers = 128; // above this, ICAO << 8 | receiver plus the 'no record' bit needs 33 bits
struct FuseArgs {
    const TrackStoreDev *bank;
    double since;                // a record contributes iff it is held and last_heard >= since
    void *keys, *skeys;          // [places] each, places = n_receivers x max_aircraft: uint32_t sort keys, uint64_t with
                                 // more than kFuseWideReceivers receivers; keys is reused after the sort
    uint32_t *vals, *svals;      // [places] each: the record's place; vals is reused as the scan's output
    uint32_t *seg_start;         // [max_fused]: where each ICAO's run starts in sorted order
    adsb_fused_aircraft *out;    // [max_fused]
    adsb_fused_level *lvl_out;   // [max_fused], or null: no fused levels (then bank->lvl is not read)
    uint64_t *counts;            // device words: [0] records written, [1] distinct ICAOs, [2] ADSB_TRACK_FUSED_TRUNCATED
    uint64_t max_fused;          // 1 .. places
    void *temp;
    size_t temp_bytes;
    uint32_t lanes;              // lanes that share one ICAO's reduction: 1 or 4
};
size_t track_fuse_temp_bytes(size_t places, uint32_t n_receivers);
hipError_t launch_track_fuse(hipStream_t s, const FuseArgs &a);

// test / measurement kernels
hipError_t launch_magnitudes(hipStream_t s, int sample_type, int mag_mode, const void *iq,
                             size_t n, uint16_t *out);
// i8: the biased squared magnitudes I^2+Q^2+72 as the nsq scan kernel's phase 1 packs them (test hook)
hipError_t launch_nsq_values(hipStream_t s, const void *iq, size_t n, uint16_t *out);
hipError_t launch_read_only(hipStream_t s, const void *buf, size_t bytes, uint32_t *sink, int shape); // shape 0..2 (kReadShapes)
constexpr int kReadShapes = 3;
hipError_t launch_synth(hipStream_t s, const adsb_synth_cfg &cfg, int sample_type,
                        uint32_t channel, uint64_t first, size_t n, void *iq);
// threads of the grid launch_synth launches (adsb_debug_synth_geometry): past it a thread writes a second sample
uint32_t synth_geometry();

} // namespace adsbk
