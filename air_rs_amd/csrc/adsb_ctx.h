// adsb_ctx.h -- what the files of the C boundary share: the context (adsb_api.cpp creates and destroys it; each feature's
// adsb_*_api.cpp reads the launch in view, launch(), and keeps its own scratch in it), the error macro, and what the others
// need from adsb_api.cpp: sync_header, and for the streaming feed (adsb_feed_api.cpp) the one-dispatch path and the view
// of an older launch.  The rule the scratch is grown by is adsb_scratch.h.  Internal.
#pragma once
#include <hip/hip_runtime.h>

#include "adsb_kernels.h"

constexpr int kTimingRing = 512;

// A device buffer of n records, grown on demand and never shrunk (adsb_scratch.h); the carved blocks count in bytes.
template <class T>
struct DevBuf {
    T *p = nullptr;
    size_t n = 0;
};

struct adsb_ctx {
    adsb_cfg cfg{};
    hipStream_t stream = nullptr;
    bool own_stream = false;
    int mag_mode = 0;
    uint32_t bps = 2; // bytes per IQ sample

    // device buffers
    void *staging = nullptr;        // host-fed input (cfg.host_staging)
    // Two result sets, used alternately: the ordering pass of launch i runs on `aux` while the
    // demod kernel of launch i+1 already runs on `stream` (they touch different sets).
    struct ResultSet {
        adsbk::Seg *seg = nullptr;       // [n_tiles_max]
        adsb_frame *slots = nullptr;     // [n_tiles_max * kQuota] fixed region, then the pool [cap_slots]
        adsb_frame *out = nullptr;       // [max_out]
        adsbk::Header *hdr = nullptr;
        uint64_t *chan_prefix = nullptr; // [max_channels + 1]: frames before each channel's first tile; last = total
        hipEvent_t k_done = nullptr, g_done = nullptr;
        bool g_pending = false;
        // the launch whose results this set holds: the one record of it.  adsb_ctx::launch() is the one in view, which
        // every fetch / re-run / levels / wire / correlate / tracker call works on (the streaming front end fetches the
        // older of two launches in flight: with_launch_in_view())
        struct Launch {
            const void *iq = nullptr;
            uint32_t channels = 0, tpc = 0, tiles = 0, cap = 0, idx = 0;
            uint64_t samples = 0, stride = 0, base = 0; // base: stream_base at the launch (re-runs of its tiles use the same)
            adsb_frame *out = nullptr;    // where the ordered list goes, [cap]
            uint64_t *hdr_pub = nullptr;  // the public 32-byte header `out` follows (ext_blob, the one-dispatch path's blob), or null
            bool valid = false;
        } li;
    } rs[2];
    hipStream_t aux = nullptr;      // ordering pass + result copies (== stream unless ADSB_OVERLAP_ORDERING=1)
    bool own_aux = false;
    adsb_packet_fields *fields = nullptr; // [max_out], allocated on first adsb_decode_fields_device_async
    bool fields_current = false;    // fields[] belongs to the last launch
    adsb_frame_level *levels = nullptr; // [max_out], allocated on first adsb_levels_device_async
    bool levels_current = false;    // levels[] belongs to the last launch
    // adsb_levels_of's own scratch (grown on demand): the records, and the device copy of a host frame list
    DevBuf<adsb_frame_level> lvof_out;
    DevBuf<adsb_frame> lvof_frames;
    // adsb_levels_modes_of's own scratch (grown on demand): the records, the device copy of a host frame list and the
    // channels' prefix
    DevBuf<adsb_frame_level> lvm_out;
    DevBuf<adsb_frame> lvm_frames;
    DevBuf<uint64_t> lvm_prefix;    // [n_channels + 1]
    bool lvm_done = false;          // a call has filled lvm_out
    uint32_t levels_blocks = 0;     // the levels kernel's largest grid: a few waves per SIMD of this device
    // wire output (adsb_wire.hip), allocated on first adsb_wire_device_async: one hipMalloc carved into the stream, the
    // frames' ends, one word per workgroup, the stream's header; and adsb_wire_of's own scratch (grown on demand) with the
    // device copies of host lists
    struct Wire {
        DevBuf<char> mem;           // the four below point into it
        uint8_t *out = nullptr;     // [44 x frames]
        uint32_t *ends = nullptr;   // [frames]
        uint32_t *block = nullptr;  // [wire_blocks(frames)]
        uint64_t *hdr = nullptr;    // {n_bytes, n_frames}
        size_t frames = 0;          // what the four hold
    } wire, wof;
    DevBuf<adsb_frame> wof_frames;
    DevBuf<adsb_frame_level> wof_levels;
    adsb_wire_cfg wire_cfg{};       // of the last adsb_wire_device_async
    bool wire_current = false;      // wire.out belongs to the last launch
    // correlate (adsb_correlate.hip), allocated on first adsb_correlate_launch / adsb_correlate_of and grown on demand:
    // one hipMalloc carved into the kernels' arrays, the receivers' prefix and bases, and device copies of host lists
    struct Corr {
        DevBuf<char> mem;           // everything in `a` below points into it
        size_t frames = 0;          // what it holds
        adsbk::CorrArgs a{};        // scratch and result pointers (frames, levels, n, ... are set per call)
        uint64_t *prefix = nullptr, *base = nullptr; // [257], [256]
        adsb_frame *in_frames = nullptr;             // [frames]
        adsb_frame_level *in_levels = nullptr;       // [frames]
        bool done = false;          // a correlate call has been enqueued
        uint32_t n = 0;             // receptions of the last call's list (what adsb_multilaterate sizes its grid by)
    } corr;
    // multilaterate (adsb_mlat.hip), allocated on first adsb_multilaterate / adsb_multilaterate_of and grown on demand:
    // one hipMalloc carved into the fixes, the reduction's temporary storage, the header and the stations; and device
    // copies of host lists
    struct Mlat {
        DevBuf<char> mem;                    // the four below point into it
        size_t msgs = 0;                     // what it holds
        adsb_mlat_fix *fixes = nullptr;      // [msgs]
        void *temp = nullptr;
        size_t temp_bytes = 0;
        adsb_mlat_header *hdr = nullptr;
        adsbk::MlatStation *stations = nullptr; // [256]
        DevBuf<adsb_message> in_msgs;        // of a host list
        DevBuf<adsb_reception> in_recs;
        DevBuf<adsb_wire_rx> in_rx;
        bool done = false;          // a multilaterate call has been enqueued
    } mlat;
    // clock sync (adsb_clock.hip), allocated on first adsb_clock_sync / adsb_clock_sync_of and grown on demand: one
    // hipMalloc carved into everything `a` below points into, and device copies of host lists
    struct Clock {
        DevBuf<char> mem;
        size_t msgs = 0, recs = 0;           // what it holds
        adsbk::ClockArgs a{};                // scratch and result pointers; the lists and the cfg of the last sync
        DevBuf<adsb_message> in_msgs;        // of a host list
        DevBuf<adsb_reception> in_recs;
        DevBuf<adsb_wire_rx> in_rx;
        bool done = false;          // a clock-sync call has been enqueued
        bool applied = false;       // ... and adsb_clock_apply behind it
    } clock;
    // wire input (adsb_wire_in.hip), allocated on first adsb_wire_in_of and grown on demand: one hipMalloc carved into the
    // kernels' arrays and the results, and the device copy of a host input
    struct WireIn {
        DevBuf<char> mem;           // everything in `a` below points into it
        size_t bytes = 0, frames = 0; // the input length and the frames it is good for
        bool levels = false;        // ... with level records
        adsbk::WireInArgs a{};      // scratch and result pointers (the input and the cfg are set per call)
        uint32_t *ends = nullptr;   // [256]
        DevBuf<uint8_t> in;         // of a host input, in whole dwords
        uint32_t n_streams = 0;     // of the last call
        bool with_levels = false;   // the last call wrote level records
        bool done = false;          // a call has been enqueued
    } win;
    // Mode S replies (adsb_modes.hip), allocated on first adsb_modes_of and grown on demand: one hipMalloc carved into
    // everything `a` below points into and the receivers' prefix, and device copies of host lists
    struct Modes {
        DevBuf<char> mem;
        size_t frames = 0, known = 0;        // what it holds: frames, and entries of known_in
        adsbk::ModesArgs a{};                // scratch and result pointers (the lists and their lengths are set per call)
        uint64_t *prefix = nullptr;          // [257]
        DevBuf<adsb_frame> in_frames;        // of a host list
        DevBuf<uint32_t> in_known;
        uint32_t n_receivers = 0;            // of the last call; 0: it had no counts
        bool done = false;                   // a call has been enqueued
    } modes;
    // Comm-B registers (adsb_commb.hip), allocated on first adsb_commb_of and grown on demand: one hipMalloc carved
    // into the partial counts, the records and the header, and the device copy of a host list
    struct Commb {
        DevBuf<char> mem;
        size_t frames = 0;                   // what it holds
        adsbk::CommbArgs a{};                // scratch and result pointers (the list and its length are set per call)
        DevBuf<adsb_frame> in_frames;        // of a host list
        bool done = false;                   // a call has been enqueued
    } commb;
    // Extended squitter status (adsb_es.hip), allocated on first adsb_es_of and grown on demand: one hipMalloc carved
    // into the partial counts, the records and the header, and the device copy of a host list
    struct Es {
        DevBuf<char> mem;
        size_t frames = 0;                   // what it holds
        adsbk::EsArgs a{};                   // scratch and result pointers (the list and its length are set per call)
        DevBuf<adsb_frame> in_frames;        // of a host list
        bool done = false;                   // a call has been enqueued
    } es;
    // Mode S replies from samples (adsb_replies.hip), allocated on first adsb_replies_of and grown on demand: one
    // hipMalloc carved into everything `a` below points into, and the device copy of a host known[]
    struct Replies {
        DevBuf<char> mem;
        size_t tiles = 0, cap = 0, channels = 0; // what it holds
        adsbk::RepliesArgs a{};              // scratch and result pointers (the samples, the cfg and known[] are set per call)
        DevBuf<uint32_t> in_known;           // of a host list
        uint32_t n_channels = 0;             // of the last call
        bool done = false;                   // a call has been enqueued
    } replies;
    // adsb_merge_lists_of's scratch (grown on demand): device copies of host lists, the channels' prefixes, and the
    // results on their way to host memory
    struct Merge {
        DevBuf<adsb_frame> a, b, out;
        DevBuf<uint32_t> src;
        DevBuf<uint64_t> prefix;             // [2 x (n_channels + 1)]
    } merge;
    // tracker (allocated on first adsb_track_device): one hipMalloc carved into the five below
    DevBuf<char> trk_mem;
    uint32_t *trk_u32 = nullptr;    // 4 x [max_out]: keys, vals, sorted keys, sorted vals
    void *trk_temp = nullptr;
    size_t trk_temp_bytes = 0;
    adsb_track_point *trk_points = nullptr;      // [max_out]
    adsb_aircraft_record *trk_aircraft = nullptr; // [max_out]
    uint64_t *trk_n_aircraft = nullptr;
    uint32_t trk_n = 0;             // frames the last tracker run covered
    bool trk_done = false;
    void *ext_blob = nullptr;       // caller-owned [32-byte header | frames] target for the next launches
    size_t ext_frames = 0;          // frame capacity of ext_blob
    bool fused_pass_only = false;   // adsb_debug_fused_pass_only (measurement)
    uint64_t stream_base = 0;       // adsb_set_stream_base: added to the offsets of the following launches
    uint32_t launch_idx = 0;        // launches so far
    uint32_t last = 0;              // result set of the launch in view: the last one, but for with_launch_in_view()
    uint32_t *out_start = nullptr;  // [n_tiles_max + 1]  (slot-overflow re-run path only)
    uint64_t *lb = nullptr;         // finish_order's exchange words: one per workgroup, then one per 64 workgroups
    uint32_t lb_groups_at = 0;
    uint32_t *scratch = nullptr;    // 16 dwords: probe result, read-kernel sink
    unsigned long long *stamps = nullptr; // cycle counters of diagnostic builds (64 bytes per tile with -DADSB_TILE_STAMPS=1)
    size_t stamps_bytes = 0;
    int scan = adsbk::kScanRoot;    // which i8 scan kernel (ADSB_SCAN=nsq selects the A/B kernel at adsb_create)
    // The one-dispatch path for small buffers (adsbk::launch_small): per result set a pinned, device-writable blob
    // [32-byte header | frames | u64 sequence number] and a device counter; a pinned input buffer for adsb_demod().
    struct Small {
        bool enabled = true, ready = false;
        char *blob[2] = {nullptr, nullptr};
        uint32_t cap = 0;            // frames per blob
        uint32_t *done = nullptr;    // device: 2 words
        char *in_host = nullptr;     // pinned copy of adsb_demod()'s buffer (allocated on first use)
        uint64_t seq = 0;
        uint64_t max_samples = 0;    // longest buffer the path takes
    } sm;
    bool pool_off = false;          // adsb_debug_pool_limit: the shared slot pool hands out nothing (test knob)
    uint32_t stall_blk = 0xFFFFFFFFu; // adsb_debug_finish_stall: this workgroup of finish_order withholds its exchange word (test knob)
    uint32_t cap_slots = 0;
    uint32_t n_tiles_max = 0;

    // pinned host mirrors
    adsbk::Header *hdr_host = nullptr;

    bool launched = false;          // a launch has been recorded: launch() describes one

    // timing
    int timing = 0;                 // 0 off; N: events on every N-th launch
    hipEvent_t ev[kTimingRing][4] = {}; // scan kernel, finishing kernel: start/end each
    bool ev_made = false;
    uint32_t ev_count = 0;

    const ResultSet::Launch &launch() const { return rs[last].li; }
    // what was derived from the list in view (decoded fields, levels, wire stream, tracker output) no longer belongs to it
    void mark_derived_stale() { fields_current = levels_current = wire_current = trk_done = false; }
    // Makes result set `set` the one in view.  Only the streaming front end looks at anything but the newest launch.
    void view_launch(uint32_t set) { last = set; mark_derived_stale(); }
};

// fn() with result set `set` in view, then the newest launch again (the next enqueue starts from the newest state)
template <class F>
int with_launch_in_view(adsb_ctx *c, uint32_t set, F fn)
{
    const uint32_t newest = c->last;
    c->view_launch(set);
    const int rc = fn();
    c->view_launch(newest);
    return rc;
}

#define HIPCHK(x)                                  \
    do {                                           \
        hipError_t e_ = (x);                       \
        if (e_ != hipSuccess) return (int)e_;      \
    } while (0)

#pragma GCC visibility push(hidden)
// Waits for the header of the launch in view in c->hdr_host (and rebuilds the list after a slot-pool overflow): adsb_api.cpp
int sync_header(adsb_ctx *c);
// The one-dispatch path for small buffers (adsb_api.cpp), as the streaming feed uses it: can a buffer take it; enqueue it;
// has result set `set`'s sequence word reached `seq`, and wait for that; complete a list whose tiles lost their slots; hand it out
bool small_fits(adsb_ctx *c, size_t n_samples);
int small_launch(adsb_ctx *c, const void *iq, size_t n_samples, uint64_t *seq_out);
bool small_reached(adsb_ctx *c, uint32_t set, uint64_t seq, bool at_least = false);
int small_wait(adsb_ctx *c, uint32_t set, uint64_t seq, bool at_least = false);
int small_complete(adsb_ctx *c, uint32_t set);
int small_collect(adsb_ctx *c, uint32_t set, adsb_frame *out, size_t max_out, size_t *n_out, uint64_t *total_found,
                  uint32_t *flags);
#pragma GCC visibility pop
