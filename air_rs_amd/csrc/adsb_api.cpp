// adsb_api.cpp -- the extern "C" boundary (include/adsb_hip.h) over the gfx950 scan kernels: the context, the launches,
// the fetch and the decoded fields.  Every other part of the boundary has a file of its own: adsb_feed_api.cpp,
// adsb_track_api.cpp, adsb_levels_api.cpp, adsb_wire_api.cpp, adsb_wire_in_api.cpp, adsb_correlate_api.cpp,
// adsb_mlat_api.cpp, adsb_clock_api.cpp.
//
// Replaces, per received buffer, the body of the reference's thread 2 loop
// (src/adsb.rs:95-116).  There is NO CPU fallback: without a HIP device adsb_create() fails with
// ADSB_E_NODEVICE and every other entry point needs a context.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "adsb_ctx.h"
#include "adsb_synth.h"

using adsbk::kTile;
using adsbk::kWindow;
using Launch = adsb_ctx::ResultSet::Launch;

static uint32_t tiles_for(uint64_t n_samples, int sample_type, int scan)
{
    if (n_samples <= (uint64_t)kWindow) return 0;
    const uint64_t n_off = n_samples - kWindow, tile = (uint64_t)adsbk::tile_offsets_of(sample_type, scan);
    return (uint32_t)((n_off + tile - 1) / tile);
}

extern "C" const char *adsb_strerror(int code)
{
    switch (code) {
    case ADSB_OK: return "ok";
    case ADSB_E_SHORT: return "buffer shorter than 240 samples (reference panics, adsb.rs:98)";
    case ADSB_E_ARG: return "bad argument";
    case ADSB_E_CAPACITY: return "exceeds the capacity the context was created with";
    case ADSB_E_NOMEM: return "out of memory";
    case ADSB_E_NODEVICE: return "no usable HIP device (there is no CPU fallback)";
    case ADSB_E_STATE: return "call sequence error";
    default: return code > 0 ? hipGetErrorString((hipError_t)code) : "unknown error";
    }
}

extern "C" void adsb_destroy(adsb_ctx *c)
{
    if (!c) return;
    (void)hipSetDevice(c->cfg.device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->ev_made)
        for (auto &e : c->ev)
            for (auto &x : e)
                if (x) (void)hipEventDestroy(x);
    if (c->own_aux && c->aux) (void)hipStreamSynchronize(c->aux);
    for (auto &r : c->rs) {
        (void)hipFree(r.seg);
        (void)hipFree(r.slots);
        (void)hipFree(r.out);
        (void)hipFree(r.hdr);
        (void)hipFree(r.chan_prefix);
        if (r.k_done) (void)hipEventDestroy(r.k_done);
        if (r.g_done) (void)hipEventDestroy(r.g_done);
    }
    void *const owned[] = {c->staging, c->out_start, c->fields, c->levels, c->lvof_out.p, c->lvof_frames.p, c->lvm_out.p,
                           c->lvm_frames.p, c->lvm_prefix.p, c->wire.mem.p,
                           c->wof.mem.p, c->wof_frames.p, c->wof_levels.p, c->corr.mem.p, c->mlat.mem.p, c->mlat.in_msgs.p,
                           c->mlat.in_recs.p, c->mlat.in_rx.p, c->clock.mem.p, c->clock.in_msgs.p, c->clock.in_recs.p,
                           c->clock.in_rx.p, c->win.mem.p, c->win.in.p, c->modes.mem.p, c->modes.in_frames.p, c->modes.in_known.p,
                           c->commb.mem.p, c->commb.in_frames.p, c->es.mem.p, c->es.in_frames.p, c->replies.mem.p,
                           c->replies.in_known.p, c->merge.a.p, c->merge.b.p, c->merge.out.p, c->merge.src.p,
                           c->merge.prefix.p, c->trk_mem.p, c->scratch,
                           c->stamps, c->lb, c->sm.done};
    for (void *p : owned) (void)hipFree(p);
    for (char *b : c->sm.blob) if (b) (void)hipHostFree(b);
    if (c->sm.in_host) (void)hipHostFree(c->sm.in_host);
    if (c->own_aux && c->aux) (void)hipStreamDestroy(c->aux);
    if (c->hdr_host) (void)hipHostFree(c->hdr_host);
    if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

// The code scan's table through the device (adsbk::launch_code_probe): tab[n] = c(n) | th(n) << 8 for n = I^2+Q^2 in
// 0 .. 32768, c = the 8-bit code the gate slides over, th = the code a "low" may reach while floor(sqrt) of a "high" n can still
// be >= its own.  What the kernel relies on (adsb_kernels.hip, "the code scan"): c is monotone, stays below 0x7C (an
// ordered f16 pattern in the high byte), and th(n) >= c(top(n)), top(n) = the largest n' with floor(sqrt(n')) = floor(sqrt(n)).
// ADSB_E_STATE if the device disagrees (no fallback: adsb_create fails).
static int code_table_check(adsb_ctx *c, uint16_t *tab)
{
    uint16_t *dev = nullptr;
    if (hipMalloc((void **)&dev, 32769 * sizeof(uint16_t)) != hipSuccess) return ADSB_E_NOMEM;
    hipError_t e = adsbk::launch_code_probe(c->stream, dev);
    if (e == hipSuccess) e = hipMemcpyAsync(tab, dev, 32769 * sizeof(uint16_t), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    (void)hipFree(dev);
    if (e != hipSuccess) return (int)e;
    uint32_t root = 0;
    for (uint32_t n = 0; n <= 32768; ++n) {
        while ((root + 1) * (root + 1) <= n) ++root;
        const uint32_t top = std::min<uint32_t>((root + 1) * (root + 1) - 1, 32768);
        const uint32_t code = tab[n] & 0xFFu, th = tab[n] >> 8, code_top = tab[top] & 0xFFu;
        if (code >= 0x7Cu || (n && code < (tab[n - 1] & 0xFFu)) || th < code_top) return ADSB_E_STATE;
    }
    return ADSB_OK;
}

extern "C" int adsb_debug_code_table(adsb_ctx *c, uint16_t *out32769)
{
    if (!c || !out32769) return ADSB_E_ARG;
    HIPCHK(hipSetDevice(c->cfg.device));
    return code_table_check(c, out32769);
}

extern "C" int adsb_create(const adsb_cfg *cfg, adsb_ctx **out_ctx)
{
    if (!cfg || !out_ctx) return ADSB_E_ARG;
    *out_ctx = nullptr;
    if (cfg->abi_version != ADSB_ABI_VERSION) return ADSB_E_ARG;
    if (cfg->sample_type != ADSB_SAMPLE_I8 && cfg->sample_type != ADSB_SAMPLE_I16) return ADSB_E_ARG;
    if (cfg->max_channels == 0 || cfg->max_samples == 0 || cfg->max_out == 0) return ADSB_E_ARG;
    if (cfg->max_out > 0x7FFFFFFFull - kTile) return ADSB_E_ARG;

    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || cfg->device < 0 || cfg->device >= ndev)
        return ADSB_E_NODEVICE;
    if (hipSetDevice(cfg->device) != hipSuccess) return ADSB_E_NODEVICE;

    adsb_ctx *c = new (std::nothrow) adsb_ctx();
    if (!c) return ADSB_E_NOMEM;
    c->cfg = *cfg;
    c->bps = cfg->sample_type == ADSB_SAMPLE_I8 ? 2 : 4;
    // i8 has two scan kernels: the product's (floor(sqrt) per sample, u8 magnitudes in LDS: eight workgroups per
    // CU) and the round-3 A/B kernel whose gate works on n = I^2+Q^2 (no root per sample, but 2 bytes of LDS per
    // sample: four workgroups per CU; 10 % fewer VALU slots, 12 % slower -- DESIGN.md section 5.3): ADSB_SCAN=nsq in
    // the environment at adsb_create selects it.
    if (const char *sp = getenv("ADSB_SMALL_PATH")) c->sm.enabled = !(sp[0] == '0');
    c->scan = adsbk::kScanRoot;
    if (const char *sc = getenv("ADSB_SCAN")) {
        if (strcmp(sc, "nsq") == 0) c->scan = adsbk::kScanNsq;
        else if (strcmp(sc, "reg") == 0) c->scan = adsbk::kScanReg;
        else if (strcmp(sc, "root") == 0 || sc[0] == 0) c->scan = adsbk::kScanRoot;
        else if (strcmp(sc, "code") == 0) c->scan = adsbk::kScanCode;
        else if (strcmp(sc, "sieve") == 0) c->scan = adsbk::kScanSieve;
        else { delete c; return ADSB_E_ARG; }
        // (the A/B kernels exist only in -DADSB_AB_KERNELS=1 builds: asking this library for one it does not have is an error)
        if (c->scan != adsbk::kScanRoot && !adsbk::ab_kernels_built()) { delete c; return ADSB_E_ARG; }
    }
    if (cfg->sample_type != ADSB_SAMPLE_I8) c->scan = adsbk::kScanRoot; // (CS16 has one scan kernel)
    uint64_t tiles = (uint64_t)tiles_for(cfg->max_samples, cfg->sample_type, c->scan) * cfg->max_channels;
    if (tiles == 0) tiles = 1;
    if (tiles * adsbk::kQuota + cfg->max_out + kTile > 0xFFFFFFF0ull) { delete c; return ADSB_E_CAPACITY; }
    c->n_tiles_max = (uint32_t)tiles;
    c->cap_slots = (uint32_t)(cfg->max_out + kTile);

    int rc = ADSB_OK;
    auto fail = [&](int code) { rc = code; };
    do {
        if (cfg->stream) {
            c->stream = (hipStream_t)cfg->stream;
        } else {
            if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { fail(ADSB_E_NODEVICE); break; }
            c->own_stream = true;
        }
        hipError_t e = hipSuccess;
        if (cfg->host_staging) {
            // +64 bytes so the staging base keeps 16-byte alignment for any channel stride rounding
            uint64_t stride = (cfg->max_samples + 7) & ~7ull;
            e = hipMalloc(&c->staging, stride * cfg->max_channels * c->bps + 64);
            if (e != hipSuccess) { fail(ADSB_E_NOMEM); break; }
        }
        // The ordering pass normally follows the demod kernel on the same stream.  Running it on its
        // own stream (ADSB_OVERLAP_ORDERING=1) lets it overlap the next launch's kernel, but measured
        // slower on MI355X: the tiny gather then competes with 16 k workgroups for CUs (26 us
        // instead of 9) and the step does not get shorter.
        const char *ov = getenv("ADSB_OVERLAP_ORDERING");
        if (ov && ov[0] == '1') {
            // (highest priority: its two small kernels should take the CU slots the scan's workgroups free, not wait
            // for the next launch's whole grid)
            int pr_lo = 0, pr_hi = 0;
            (void)hipDeviceGetStreamPriorityRange(&pr_lo, &pr_hi);
            if (hipStreamCreateWithPriority(&c->aux, hipStreamNonBlocking, pr_hi) != hipSuccess) { fail(ADSB_E_NODEVICE); break; }
            c->own_aux = true;
        } else {
            c->aux = c->stream;
        }
        const size_t n_slots = (size_t)c->n_tiles_max * adsbk::kQuota + c->cap_slots;
        bool ok = true;
        for (auto &r : c->rs) {
            ok = ok && hipMalloc((void **)&r.seg, sizeof(adsbk::Seg) * (size_t)c->n_tiles_max) == hipSuccess &&
                 hipMalloc((void **)&r.slots, sizeof(adsb_frame) * n_slots) == hipSuccess &&
                 hipMalloc((void **)&r.out, sizeof(adsb_frame) * (size_t)cfg->max_out) == hipSuccess &&
                 hipMalloc((void **)&r.hdr, sizeof(adsbk::Header)) == hipSuccess &&
                 hipMalloc((void **)&r.chan_prefix, sizeof(uint64_t) * ((size_t)cfg->max_channels + 1)) == hipSuccess &&
                 hipMemsetAsync(r.chan_prefix, 0, sizeof(uint64_t) * ((size_t)cfg->max_channels + 1), c->stream) == hipSuccess &&
                 hipEventCreateWithFlags(&r.k_done, hipEventDisableTiming | hipEventReleaseToDevice) == hipSuccess &&
                 hipEventCreateWithFlags(&r.g_done, hipEventDisableTiming | hipEventReleaseToDevice) == hipSuccess &&
                 hipMemsetAsync(r.hdr, 0, sizeof(adsbk::Header), c->stream) == hipSuccess;
        }
        c->lb_groups_at = (uint32_t)(((size_t)c->n_tiles_max / adsbk::kFinishTilesPerWg + 2 + 63) / 64 * 64);
        const size_t lb_words = (size_t)c->lb_groups_at + c->lb_groups_at / 64 + 64;
        ok = ok && hipMalloc((void **)&c->out_start, sizeof(uint32_t) * ((size_t)c->n_tiles_max + 1)) == hipSuccess &&
             hipMalloc((void **)&c->scratch, 64) == hipSuccess &&
             hipMalloc((void **)&c->lb, sizeof(uint64_t) * lb_words) == hipSuccess &&
             hipMemsetAsync(c->lb, 0, sizeof(uint64_t) * lb_words, c->stream) == hipSuccess &&
             hipMemsetAsync(c->scratch, 0, 64, c->stream) == hipSuccess;
        if (!ok) { fail(ADSB_E_NOMEM); break; }
        if (hipHostMalloc((void **)&c->hdr_host, sizeof(adsbk::Header), hipHostMallocDefault) != hipSuccess) { fail(ADSB_E_NOMEM); break; }
        uint32_t probe[4] = {0, 0, 0, 0};
        e = adsbk::probe_cvt(c->stream, c->scratch, probe);
        if (e != hipSuccess) { fail((int)e); break; }
        // expected truncation of {0.75, 2.5, 180.9986} = {0, 2, 180}
        const uint32_t want = 0u | (2u << 8) | (180u << 16);
        if (probe[0] == want) c->mag_mode = 0;
        else if (probe[1] == want) c->mag_mode = 1;
        else c->mag_mode = 2;
        if (const char *force = getenv("ADSB_FORCE_MAG_MODE")) c->mag_mode = atoi(force) % 3;
        if (c->scan == adsbk::kScanCode) {
            // The code scan's gate is a SUPERSET test only if this device's conversion and f16 multiply-add behave as the
            // kernel assumes: check it through the kernel's own instructions, for every n an i8 sample can give.
            std::vector<uint16_t> tab(32769);
            const int prc = code_table_check(c, tab.data());
            if (prc != ADSB_OK) { fail(prc); break; }
        }
        // cycle counters of diagnostic builds (-DADSB_TILE_STAMPS=1); zeros otherwise
        c->stamps_bytes = adsbk::tile_stamps_built() ? (size_t)c->n_tiles_max * 64 + 512 : 512;
        if (hipMalloc((void **)&c->stamps, c->stamps_bytes) != hipSuccess || hipMemsetAsync(c->stamps, 0, c->stamps_bytes, c->stream) != hipSuccess) { fail(ADSB_E_NOMEM); break; }
    } while (0);
    if (rc != ADSB_OK) { adsb_destroy(c); return rc; }
    *out_ctx = c;
    return ADSB_OK;
}

extern "C" void *adsb_stream(adsb_ctx *c) { return c ? (void *)c->stream : nullptr; }
extern "C" int adsb_sample_type(const adsb_ctx *c) { return c ? c->cfg.sample_type : ADSB_E_ARG; }
extern "C" int adsb_debug_fused_pass_only(adsb_ctx *c, int on)
{
    if (!c) return ADSB_E_ARG;
    c->fused_pass_only = on != 0;
    return ADSB_OK;
}
extern "C" int adsb_debug_mag_mode(adsb_ctx *c) { return c ? c->mag_mode : ADSB_E_ARG; }
extern "C" int adsb_debug_scan(adsb_ctx *c) { return c ? (c->cfg.sample_type == ADSB_SAMPLE_I8 ? c->scan : adsbk::kScanRoot) : ADSB_E_ARG; }
// Test knobs.  adsb_debug_set_launch_index: the next launch counts as launch number `idx` (the exchange words' epoch is
// derived from it: lets a test cross the 2^30 wrap).  adsb_debug_finish_stall: finish_order's workgroup `blk` of the
// following launches withholds its exchange word (0xFFFFFFFF: none) -- the workgroups behind it give up after ~0.1 s.
extern "C" int adsb_debug_set_launch_index(adsb_ctx *c, uint32_t idx)
{
    if (!c) return ADSB_E_ARG;
    HIPCHK(hipSetDevice(c->cfg.device));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (c->own_aux) HIPCHK(hipStreamSynchronize(c->aux));
    c->launch_idx = idx;
    return ADSB_OK;
}
extern "C" int adsb_debug_finish_stall(adsb_ctx *c, uint32_t blk)
{
    if (!c) return ADSB_E_ARG;
    c->stall_blk = blk;
    return ADSB_OK;
}

extern "C" int adsb_debug_pool_limit(adsb_ctx *c, int on)
{
    if (!c) return ADSB_E_ARG;
    c->pool_off = on != 0;
    return ADSB_OK;
}

extern "C" int adsb_debug_finish_geometry(uint32_t *tiles_per_workgroup, uint32_t *fan, uint32_t *flat, uint32_t *sums_per_round)
{
    adsbk::finish_geometry(tiles_per_workgroup, fan, flat, sums_per_round);
    return ADSB_OK;
}

extern "C" int adsb_debug_tile_stamps(adsb_ctx *c, uint32_t *out, size_t max_tiles, size_t *n_tiles)
{
    if (!c || !n_tiles || (!out && max_tiles)) return ADSB_E_ARG;
    if (!adsbk::tile_stamps_built() || !c->stamps) return ADSB_E_STATE;
    HIPCHK(hipSetDevice(c->cfg.device));
    HIPCHK(hipStreamSynchronize(c->stream));
    const size_t n = std::min<size_t>(max_tiles, c->launch().tiles);
    if (n) HIPCHK(hipMemcpy(out, c->stamps, n * 64, hipMemcpyDeviceToHost));
    *n_tiles = n;
    return ADSB_OK;
}

// Records in result set `r` what launch `idx` works on, before any argument struct is built from it; the derived results
// are stale from here.  The list goes behind the public header `hdr_pub` ([32 bytes | cap frames]) or, without one, to the
// set's own `out`.  The launch becomes the one in view (and li.valid) only when every enqueue has succeeded.
static Launch &record_launch(adsb_ctx *c, adsb_ctx::ResultSet &r, uint32_t idx, const void *iq, uint32_t channels,
                             uint64_t samples, uint64_t stride, void *hdr_pub, uint32_t cap)
{
    Launch &li = r.li;
    li.valid = false;
    li.iq = iq;
    li.channels = channels;
    li.samples = samples;
    li.stride = stride;
    li.base = c->stream_base;
    li.tpc = tiles_for(samples, c->cfg.sample_type, c->scan);
    li.tiles = li.tpc * channels;
    li.out = hdr_pub ? reinterpret_cast<adsb_frame *>(static_cast<char *>(hdr_pub) + 32) : r.out;
    li.cap = cap;
    li.hdr_pub = static_cast<uint64_t *>(hdr_pub);
    li.idx = idx;
    c->launched = true;
    c->mark_derived_stale();
    return li;
}

// (both read the launch from r.li: the first pass publishes the public header, a re-run of lost tiles does not)
static adsbk::DemodArgs demod_args(adsb_ctx *c, adsb_ctx::ResultSet &r, uint32_t tile_first, uint32_t tile_count,
                                   bool first_pass)
{
    adsbk::DemodArgs a{};
    a.iq = r.li.iq;
    a.n_samples = r.li.samples;
    a.channel_stride = r.li.stride;
    a.tiles_per_channel = r.li.tpc;
    a.tile_first = tile_first;
    a.tile_count = tile_count;
    a.count_groups = first_pass ? 1u : 0u;
    a.offset_base = r.li.base;
    a.fused_pass_only = c->fused_pass_only ? 1u : 0u;
    a.seg = r.seg;
    a.slots = r.slots;
    a.pool_first = c->n_tiles_max * adsbk::kQuota;
    a.cap_slots = c->cap_slots;
    a.hdr = r.hdr;
    a.hdr_pub = first_pass ? r.li.hdr_pub : nullptr;
    a.pool_off = (c->pool_off && first_pass) ? 1u : 0u; // (first passes only: the re-run of lost tiles needs the pool)
    a.stamps = c->stamps;
    return a;
}

static adsbk::FinishArgs finish_args(adsb_ctx *c, adsb_ctx::ResultSet &r, uint32_t tile_first, uint32_t tile_count, bool rerun)
{
    adsbk::FinishArgs a{};
    a.seg = r.seg;
    a.slots = r.slots;
    a.out_start = rerun ? c->out_start : nullptr;
    a.lb = c->lb;
    a.lb_groups_at = c->lb_groups_at;
    a.chan_prefix = rerun ? nullptr : r.chan_prefix;
    a.epoch = (r.li.idx + 1u) & 0x3FFFFFFFu; // (the index of the launch the pass belongs to tags the look-back words)
    a.out = r.li.out;
    a.hdr_pub = rerun ? nullptr : r.li.hdr_pub;
    a.tiles_per_channel = r.li.tpc;
    a.n_channels = r.li.channels;
    a.max_out = r.li.cap;
    a.tile_first = tile_first;
    a.tile_count = tile_count;
    a.hdr = r.hdr;
    a.stall_blk = rerun ? 0xFFFFFFFFu : c->stall_blk;
    return a;
}

// finish_order's exchange words are never cleared: they carry the launch's 30-bit epoch ((launch index + 1) mod 2^30) and a
// word of another epoch reads as "not there yet".  A word written exactly 2^30 launches ago would read as this launch's:
// whenever the epoch wraps (every ~4 hours of back-to-back 13 us launches) the words are zeroed on the stream first.
static hipError_t clear_exchange_words_at_wrap(adsb_ctx *c, uint32_t launch_idx)
{
    if (((launch_idx + 1u) & 0x3FFFFFFFu) != 0u) return hipSuccess;
    const size_t lb_words = (size_t)c->lb_groups_at + c->lb_groups_at / 64 + 64;
    return hipMemsetAsync(c->lb, 0, sizeof(uint64_t) * lb_words, c->aux);
}

extern "C" int adsb_demod_device_async(adsb_ctx *c, const void *iq_dev, uint32_t n_channels,
                                       size_t n_samples, size_t channel_stride)
{
    if (!c || !iq_dev || n_channels == 0) return ADSB_E_ARG;
    if (n_samples < (size_t)kWindow) return ADSB_E_SHORT;
    if (n_channels > c->cfg.max_channels || n_samples > c->cfg.max_samples) return ADSB_E_CAPACITY;
    if (((uintptr_t)iq_dev & 15u) != 0) return ADSB_E_ARG;
    if (n_channels > 1 && (channel_stride < n_samples || (channel_stride & 7u) != 0)) return ADSB_E_ARG;
    if (n_channels == 1) channel_stride = n_samples;
    HIPCHK(hipSetDevice(c->cfg.device));

    // Launch i uses result set i & 1.  (ADSB_OVERLAP_ORDERING=1: the finishing kernel of launch i runs on `aux` beside
    // the scan of launch i+1, which only has to wait for the finishing kernel of launch i-2: same result set.)
    const uint32_t i = c->launch_idx;
    adsb_ctx::ResultSet &r = c->rs[i & 1u];
    const Launch &li = record_launch(c, r, i, iq_dev, n_channels, n_samples, channel_stride, c->ext_blob,
                                     (uint32_t)std::min<size_t>(c->ext_blob ? c->ext_frames : c->cfg.max_out, c->cfg.max_out));
    if (c->own_aux && r.g_pending) HIPCHK(hipStreamWaitEvent(c->stream, r.g_done, 0));
    HIPCHK(clear_exchange_words_at_wrap(c, i));

    hipEvent_t *ev = nullptr;
    if (c->timing && (c->launch_idx % (uint32_t)c->timing) == 0) {
        if (!c->ev_made) {
            for (auto &e : c->ev)
                for (auto &x : e) HIPCHK(hipEventCreateWithFlags(&x, hipEventReleaseToDevice)); // no system-scope flush
            c->ev_made = true;
        }
        ev = c->ev[c->ev_count % kTimingRing];
    }
    const adsbk::DemodArgs da = demod_args(c, r, 0, li.tiles, true);
    // (ADSB_OVERLAP_ORDERING=1: the event the other stream waits for rides on the scan's own dispatch packet: no
    // barrier packet between two scans.)
    hipEvent_t scan_done = ev ? ev[1] : (c->own_aux ? r.k_done : nullptr);
    HIPCHK(adsbk::launch_demod(c->stream, c->cfg.sample_type, c->mag_mode, c->scan, da, ev ? ev[0] : nullptr, scan_done));
    if (c->own_aux && scan_done && li.tiles) HIPCHK(hipStreamWaitEvent(c->aux, scan_done, 0));
    // second kernel: CRC-24 / repair of the survivors the scan kernel sliced, and the ordered list.  Without tiles
    // (exactly 240 samples: adsb.rs:98 iterates 0..0) or in measurement mode (scan only) the list is empty.
    if (li.tiles == 0 || c->fused_pass_only) {
        HIPCHK(adsbk::launch_empty_result(c->aux, r.hdr, li.hdr_pub, r.chan_prefix, li.channels, ev ? ev[2] : nullptr,
                                          ev ? ev[3] : nullptr));
    } else {
        HIPCHK(adsbk::launch_finish(c->aux, finish_args(c, r, 0, li.tiles, false), ev ? ev[2] : nullptr, ev ? ev[3] : nullptr));
    }
    // (same stream: in-order already; adsb_stream_wait_results records the event when somebody asks for it)
    if (c->own_aux) {
        HIPCHK(hipEventRecord(r.g_done, c->aux));
        r.g_pending = true;
    }
    c->last = i & 1u;
    r.li.valid = true;
    c->launch_idx = i + 1u;
    if (ev && li.tiles) c->ev_count++;
    return ADSB_OK;
}

// ---- the one-dispatch path for small buffers --------------------------------------------------------------------------
// (adsbk::demod_small: every workgroup scans its tile, the last one to finish checks and orders all survivors and writes
// header + frames straight into pinned host memory, then a sequence number the host polls.)  One HIP call per buffer
// instead of a copy, three launches, two result copies and their synchronisations: what the reference's own buffer sizes
// (20 000 samples, adsb.rs:77-79; MTU-sized reads, adsb.rs:59-64) need.
static size_t small_blob_bytes(uint32_t cap) { return 32 + sizeof(adsb_frame) * (size_t)cap + 16; }
static uint64_t *small_seq_word(adsb_ctx *c, uint32_t set)
{
    return reinterpret_cast<uint64_t *>(c->sm.blob[set] + 32 + sizeof(adsb_frame) * (size_t)c->sm.cap);
}

static int small_init(adsb_ctx *c)
{
    if (c->sm.ready) return ADSB_OK;
    if (!c->sm.enabled) return ADSB_E_STATE;
    const uint64_t tile = (uint64_t)adsbk::tile_offsets_of(c->cfg.sample_type, c->scan);
    c->sm.max_samples = std::min<uint64_t>(c->cfg.max_samples, tile * adsbk::kFinishTilesPerWg + kWindow);
    // a buffer of n samples has at most n - 240 frames (one per offset: SURVEY F8)
    c->sm.cap = (uint32_t)std::min<uint64_t>(c->cfg.max_out, c->sm.max_samples);
    if (c->sm.cap == 0) return ADSB_E_STATE;
    HIPCHK(hipSetDevice(c->cfg.device));
    for (int k = 0; k < 2; ++k) {
        // coherent (fine-grained) host memory: the device's writes are visible to the polling host while the stream runs
        if (hipHostMalloc((void **)&c->sm.blob[k], small_blob_bytes(c->sm.cap), hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) {
            (void)hipGetLastError();
            c->sm.enabled = false;
            return ADSB_E_NOMEM;
        }
        std::memset(c->sm.blob[k], 0, 32);
        *small_seq_word(c, (uint32_t)k) = 0;
    }
    if (hipMalloc((void **)&c->sm.done, 2 * sizeof(uint32_t)) != hipSuccess ||
        hipMemsetAsync(c->sm.done, 0, 2 * sizeof(uint32_t), c->stream) != hipSuccess) {
        c->sm.enabled = false;
        return ADSB_E_NOMEM;
    }
    c->sm.ready = true;
    return ADSB_OK;
}

// Can this buffer take the one-dispatch path?  (Not while the caller redirects results into a blob of its own.)
bool small_fits(adsb_ctx *c, size_t n_samples)
{
    return c->sm.enabled && !c->ext_blob && !c->fused_pass_only && !c->own_aux && n_samples > (size_t)kWindow &&
           small_init(c) == ADSB_OK && n_samples <= c->sm.max_samples;
}

// Enqueues one buffer (device-visible memory: pinned host or device, 16-byte aligned) as launch `launch_idx`; like
// adsb_demod_device_async for one channel, in one dispatch.  *seq_out = the value the blob's sequence word will carry.
int small_launch(adsb_ctx *c, const void *iq, size_t n_samples, uint64_t *seq_out)
{
    HIPCHK(hipSetDevice(c->cfg.device));
    const uint32_t i = c->launch_idx, set = i & 1u;
    adsb_ctx::ResultSet &r = c->rs[set];
    const uint32_t tiles = record_launch(c, r, i, iq, 1, n_samples, n_samples, c->sm.blob[set], c->sm.cap).tiles;
    HIPCHK(clear_exchange_words_at_wrap(c, i));
    const adsbk::DemodArgs da = demod_args(c, r, 0, tiles, true);
    const adsbk::FinishArgs fa = finish_args(c, r, 0, tiles, false);
    adsbk::SmallArgs sa{};
    sa.done = c->sm.done + set;
    sa.seq_host = small_seq_word(c, set);
    sa.seq = ++c->sm.seq;
    HIPCHK(adsbk::launch_small(c->stream, c->cfg.sample_type, c->mag_mode, c->scan, da, fa, sa));
    c->last = i & 1u;
    r.li.valid = true;
    c->launch_idx = i + 1u;
    *seq_out = sa.seq;
    return ADSB_OK;
}

// Does result set `set` carry sequence number `seq`?  (at_least: a LATER launch on the same result set has finished -- the
// stream is in order -- will do as well: used where only "the device no longer reads that launch's input" matters)
bool small_reached(adsb_ctx *c, uint32_t set, uint64_t seq, bool at_least)
{
    const uint64_t v = __atomic_load_n(small_seq_word(c, set), __ATOMIC_ACQUIRE);
    return at_least ? v >= seq : v == seq;
}

// Waits (polling pinned memory, no HIP call on the usual path) until it does.
int small_wait(adsb_ctx *c, uint32_t set, uint64_t seq, bool at_least)
{
    for (uint32_t spins = 0; !small_reached(c, set, seq, at_least); ++spins) {
        if (spins > (1u << 22)) { // ~ tens of milliseconds of polling: let the runtime tell what happened
            HIPCHK(hipSetDevice(c->cfg.device));
            HIPCHK(hipStreamSynchronize(c->stream));
            if (!small_reached(c, set, seq, at_least)) return ADSB_E_STATE;
            break;
        }
#if defined(__x86_64__)
        __builtin_ia32_pause();
#endif
    }
    return ADSB_OK;
}

// Completes the list of result set `set` (a small launch that small_wait has seen complete) if tiles of it lost their
// slots: the re-run scans the launch's samples (li.iq) AGAIN, so they must still be where the launch read them.  Leaves
// the newest launch the one in view.
int small_complete(adsb_ctx *c, uint32_t set)
{
    const uint64_t *hdr = reinterpret_cast<const uint64_t *>(c->sm.blob[set]);
    if (!(hdr[2] & ADSB_FLAG_INCOMPLETE)) return ADSB_OK;
    // slot-pool overflow (pathological input): the standard re-run path completes the blob in place
    const int rc = with_launch_in_view(c, set, [&] { return sync_header(c); });
    if (rc != ADSB_OK) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));
    return ADSB_OK;
}

// Hands the finished list of result set `set` (a small launch that small_wait has seen complete) to the caller.
int small_collect(adsb_ctx *c, uint32_t set, adsb_frame *out, size_t max_out, size_t *n_out, uint64_t *total_found,
                  uint32_t *flags)
{
    const uint64_t *hdr = reinterpret_cast<const uint64_t *>(c->sm.blob[set]);
    int rc = small_complete(c, set);
    if (rc != ADSB_OK) return rc;
    uint64_t n = hdr[0];
    uint32_t fl = (uint32_t)hdr[2] & ~ADSB_FLAG_INCOMPLETE;
    if (n > max_out) { n = max_out; fl |= ADSB_FLAG_TRUNCATED; }
    if (n) std::memcpy(out, c->sm.blob[set] + 32, sizeof(adsb_frame) * (size_t)n);
    *n_out = (size_t)n;
    if (total_found) *total_found = hdr[1];
    if (flags) *flags = fl;
    return ADSB_OK;
}

// Slot-pool overflow (far more gate survivors than max_out + one tile): redo the tiles that feed
// the first max_out frames in batches whose survivors fit.  Counts from the first pass are exact,
// so the plan is made on the host.  Only pathological inputs get here.
static int rerun_in_batches(adsb_ctx *c, adsb_ctx::ResultSet &r)
{
    HIPCHK(hipStreamSynchronize(c->aux));
    HIPCHK(hipStreamSynchronize(c->stream));
    const uint32_t n = r.li.tiles;
    std::vector<adsbk::Seg> seg(n);
    HIPCHK(hipMemcpyAsync(seg.data(), r.seg, sizeof(adsbk::Seg) * n, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    std::vector<uint32_t> start((size_t)n + 1);
    uint64_t run = 0;
    for (uint32_t t = 0; t <= n; ++t) {
        start[t] = run > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)run;
        if (t < n) run += seg[t].valid;
    }
    HIPCHK(hipMemcpyAsync(c->out_start, start.data(), sizeof(uint32_t) * ((size_t)n + 1), hipMemcpyHostToDevice, c->stream));
    uint32_t limit = 0;
    while (limit < n && start[limit] < r.li.cap) ++limit;
    uint32_t t0 = 0;
    int rc = ADSB_OK;
    while (t0 < limit && rc == ADSB_OK) {
        uint64_t used = 0;
        uint32_t t1 = t0;
        auto pool_need = [&](uint32_t t) { return seg[t].cand > adsbk::kQuota ? (uint64_t)seg[t].cand : 0ull; };
        while (t1 < limit && used + pool_need(t1) <= c->cap_slots) used += pool_need(t1++);
        if (t1 == t0) { rc = ADSB_E_STATE; break; } // a single tile never exceeds cap_slots (>= kTile)
        hipError_t e;
        if ((e = hipMemsetAsync(&r.hdr->alloc, 0, sizeof(unsigned long long), c->stream)) != hipSuccess ||
            (e = adsbk::launch_demod(c->stream, c->cfg.sample_type, c->mag_mode, c->scan,
                                     demod_args(c, r, t0, t1 - t0, false))) != hipSuccess ||
            (e = adsbk::launch_finish(c->stream, finish_args(c, r, t0, t1 - t0, true))) != hipSuccess)
            rc = (int)e;
        t0 = t1;
    }
    HIPCHK(hipMemsetAsync(&r.hdr->alloc, 0, sizeof(unsigned long long), c->stream));
    HIPCHK(hipMemsetAsync(&r.hdr->retry, 0, sizeof(uint32_t), c->stream));
    if (rc == ADSB_OK) { // the list is whole now: drop ADSB_FLAG_INCOMPLETE where device-side consumers read it
        c->hdr_host->flags &= ~ADSB_FLAG_INCOMPLETE;
        const uint64_t pub_flags = c->hdr_host->flags;
        HIPCHK(hipMemcpyAsync(&r.hdr->flags, &c->hdr_host->flags, sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
        if (r.li.hdr_pub) // the launch wrote into a blob: [n_out | total | flags | 0 | frames]
            HIPCHK(hipMemcpyAsync(r.li.hdr_pub + 2, &pub_flags, sizeof(uint64_t), hipMemcpyDefault, c->stream)); // (the blob may be pinned host memory: the small-buffer path)
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    return rc;
}

int sync_header(adsb_ctx *c)
{
    if (!c->launched) return ADSB_E_STATE;
    HIPCHK(hipSetDevice(c->cfg.device));
    adsb_ctx::ResultSet &r = c->rs[c->last];
    HIPCHK(hipMemcpyAsync(c->hdr_host, r.hdr, sizeof(adsbk::Header), hipMemcpyDeviceToHost, c->aux));
    HIPCHK(hipStreamSynchronize(c->aux)); // the ordering pass of the last launch ran on aux before this copy
    if (c->hdr_host->retry & 4u) return ADSB_E_STATE; // finish_order gave up waiting for a workgroup (never seen; see its comment)
    if (c->hdr_host->retry) {
        int rc = rerun_in_batches(c, r);
        if (rc != ADSB_OK) return rc;
        c->hdr_host->retry = 0;
        c->mark_derived_stale(); // the list was rebuilt
    }
    return ADSB_OK;
}

extern "C" int adsb_fetch_counts(adsb_ctx *c, uint64_t *n_out, uint64_t *total_found, uint32_t *flags)
{
    if (!c) return ADSB_E_ARG;
    int rc = sync_header(c);
    if (rc != ADSB_OK) return rc;
    if (n_out) *n_out = c->hdr_host->n_out;
    if (total_found) *total_found = c->hdr_host->total_found;
    if (flags) *flags = c->hdr_host->flags;
    return ADSB_OK;
}

extern "C" int adsb_fetch(adsb_ctx *c, adsb_frame *out, size_t max_out, size_t *n_out,
                          uint64_t *per_channel_counts, uint64_t *total_found, uint32_t *flags)
{
    if (!c || !n_out || (!out && max_out)) return ADSB_E_ARG;
    int rc = sync_header(c);
    if (rc != ADSB_OK) return rc;
    uint64_t n = c->hdr_host->n_out;
    uint32_t fl = c->hdr_host->flags;
    if (n > max_out) { n = max_out; fl |= ADSB_FLAG_TRUNCATED; }
    adsb_ctx::ResultSet &r = c->rs[c->last];
    if (n) HIPCHK(hipMemcpyAsync(out, c->launch().out, sizeof(adsb_frame) * n, hipMemcpyDefault, c->aux)); // (device memory, or the small-buffer path's pinned blob)
    std::vector<uint64_t> pre;
    if (per_channel_counts) {
        pre.resize((size_t)c->launch().channels + 1);
        HIPCHK(hipMemcpyAsync(pre.data(), r.chan_prefix, sizeof(uint64_t) * pre.size(), hipMemcpyDeviceToHost, c->aux));
    }
    HIPCHK(hipStreamSynchronize(c->aux));
    if (per_channel_counts) { // frames of channel k in `out` = its share of the first n frames of the list
        for (uint32_t k = 0; k < c->launch().channels; ++k)
            per_channel_counts[k] = std::min<uint64_t>(pre[k + 1], n) - std::min<uint64_t>(pre[k], n);
    }
    *n_out = (size_t)n;
    if (total_found) *total_found = c->hdr_host->total_found;
    if (flags) *flags = fl;
    return ADSB_OK;
}

extern "C" int adsb_result_device(adsb_ctx *c, const adsb_frame **frames_dev, const void **header_dev)
{
    if (!c) return ADSB_E_ARG;
    if (frames_dev) *frames_dev = c->launch().out ? c->launch().out : c->rs[c->last].out;
    if (header_dev) *header_dev = c->rs[c->last].hdr;
    return ADSB_OK;
}

extern "C" int adsb_decode_fields_device_async(adsb_ctx *c)
{
    if (!c) return ADSB_E_ARG;
    if (!c->launched) return ADSB_E_STATE;
    HIPCHK(hipSetDevice(c->cfg.device));
    if (!c->fields && hipMalloc((void **)&c->fields, sizeof(adsb_packet_fields) * (size_t)c->cfg.max_out) != hipSuccess)
        return ADSB_E_NOMEM;
    // same stream as the ordering pass, so it sees the finished list and header
    HIPCHK(adsbk::launch_decode_fields(c->aux, c->launch().out, c->rs[c->last].hdr, c->launch().cap, c->fields));
    c->fields_current = true;
    return ADSB_OK;
}

extern "C" int adsb_fields_device(adsb_ctx *c, const adsb_packet_fields **fields_dev)
{
    if (!c || !fields_dev) return ADSB_E_ARG;
    *fields_dev = c->fields;
    return c->fields ? ADSB_OK : ADSB_E_STATE;
}

extern "C" int adsb_fetch_fields(adsb_ctx *c, adsb_packet_fields *out, size_t max_out, size_t *n_out)
{
    if (!c || !n_out || (!out && max_out)) return ADSB_E_ARG;
    if (!c->fields) return ADSB_E_STATE;
    int rc = sync_header(c);
    if (rc != ADSB_OK) return rc;
    uint64_t n = std::min<uint64_t>(c->hdr_host->n_out, c->launch().cap);
    if (n > max_out) n = max_out;
    if (n) HIPCHK(hipMemcpyAsync(out, c->fields, sizeof(adsb_packet_fields) * n, hipMemcpyDeviceToHost, c->aux));
    HIPCHK(hipStreamSynchronize(c->aux));
    *n_out = (size_t)n;
    return ADSB_OK;
}

extern "C" int adsb_set_result_target(adsb_ctx *c, void *blob_dev, size_t blob_bytes)
{
    if (!c) return ADSB_E_ARG;
    if (!blob_dev) { c->ext_blob = nullptr; c->ext_frames = 0; return ADSB_OK; }
    if (((uintptr_t)blob_dev & 15u) || blob_bytes < 32 + sizeof(adsb_frame)) return ADSB_E_ARG;
    c->ext_blob = blob_dev;
    c->ext_frames = (blob_bytes - 32) / sizeof(adsb_frame);
    return ADSB_OK;
}

extern "C" int adsb_set_stream_base(adsb_ctx *c, uint64_t first_sample_index)
{
    if (!c) return ADSB_E_ARG;
    c->stream_base = first_sample_index;
    return ADSB_OK;
}

extern "C" int adsb_stream_wait_results(adsb_ctx *c, void *stream)
{
    if (!c) return ADSB_E_ARG;
    if (!c->launched) return ADSB_E_STATE;
    HIPCHK(hipSetDevice(c->cfg.device));
    if (!c->own_aux) HIPCHK(hipEventRecord(c->rs[c->last].g_done, c->aux)); // tail of the in-order stream
    HIPCHK(hipStreamWaitEvent((hipStream_t)stream, c->rs[c->last].g_done, 0));
    return ADSB_OK;
}

extern "C" int adsb_demod(adsb_ctx *c, const void *iq, size_t n_samples, adsb_frame *out,
                          size_t max_out, size_t *n_out, uint32_t *flags)
{
    if (!c || !iq || !n_out) return ADSB_E_ARG;
    *n_out = 0;
    if (flags) *flags = 0;
    if (!c->staging) return ADSB_E_STATE;
    if (n_samples < (size_t)kWindow) return ADSB_E_SHORT;
    if (n_samples > c->cfg.max_samples) return ADSB_E_CAPACITY;
    HIPCHK(hipSetDevice(c->cfg.device));
    if (small_fits(c, n_samples)) {
        // a small buffer (the reference's own sizes): copy it into pinned memory the device reads directly, ONE dispatch,
        // the frames come back through pinned memory too -- no copy commands, no stream synchronisation
        if (!c->sm.in_host &&
            hipHostMalloc((void **)&c->sm.in_host, (size_t)c->sm.max_samples * c->bps + 64, hipHostMallocMapped) != hipSuccess) {
            (void)hipGetLastError();
            c->sm.enabled = false;
        } else {
            std::memcpy(c->sm.in_host, iq, n_samples * c->bps);
            uint64_t seq = 0;
            int rc = small_launch(c, c->sm.in_host, n_samples, &seq);
            if (rc != ADSB_OK) return rc;
            const uint32_t set = c->last;
            rc = small_wait(c, set, seq);
            if (rc != ADSB_OK) return rc;
            return small_collect(c, set, out, max_out, n_out, nullptr, flags);
        }
    }
    HIPCHK(hipMemcpyAsync(c->staging, iq, n_samples * c->bps, hipMemcpyHostToDevice, c->stream));
    int rc = adsb_demod_device_async(c, c->staging, 1, n_samples, n_samples);
    if (rc != ADSB_OK) return rc;
    return adsb_fetch(c, out, max_out, n_out, nullptr, nullptr, flags);
}

// ---- measurement / test helpers -----------------------------------------------------------------
extern "C" int adsb_timing_enable(adsb_ctx *c, int on)
{
    if (!c) return ADSB_E_ARG;
    c->timing = on > 0 ? on : 0;
    c->ev_count = 0;
    return ADSB_OK;
}

static int timing_read(adsb_ctx *c, double *demod_ms, double *order_ms, double *decode_ms, uint32_t *n_launches);
extern "C" int adsb_timing_read(adsb_ctx *c, double *demod_ms, double *order_ms, uint32_t *n_launches)
{
    return timing_read(c, demod_ms, order_ms, nullptr, n_launches);
}
extern "C" int adsb_timing_read3(adsb_ctx *c, double *scan_ms, double *decode_ms, double *order_ms, uint32_t *n_launches)
{
    return timing_read(c, scan_ms, order_ms, decode_ms, n_launches);
}
static int timing_read(adsb_ctx *c, double *demod_ms, double *order_ms, double *decode_ms, uint32_t *n_launches)
{
    if (!c) return ADSB_E_ARG;
    HIPCHK(hipSetDevice(c->cfg.device));
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipStreamSynchronize(c->aux));
    uint32_t n = std::min<uint32_t>(c->ev_count, kTimingRing);
    double a = 0, b = 0;
    for (uint32_t k = 0; k < n; ++k) {
        float x = 0, y = 0;
        HIPCHK(hipEventElapsedTime(&x, c->ev[k][0], c->ev[k][1]));
        HIPCHK(hipEventElapsedTime(&y, c->ev[k][2], c->ev[k][3]));
        a += x;
        b += y;
    }
    // a launch is two kernels since round 3: the scan and finish_order (CRC / repair + the ordered list in one); the
    // latter is reported as the "decode" figure, the separate ordering pass no longer exists (0)
    if (demod_ms) *demod_ms = n ? a / n : 0.0;
    if (decode_ms) *decode_ms = n ? b / n : 0.0;
    if (order_ms) *order_ms = decode_ms ? 0.0 : (n ? b / n : 0.0);
    if (n_launches) *n_launches = n;
    c->ev_count = 0;
    return ADSB_OK;
}

extern "C" int adsb_time_read_ceiling(adsb_ctx *c, const void *buf_dev, size_t bytes, int iters,
                                      double *ms_per_pass)
{
    if (!c || !buf_dev || iters <= 0 || !ms_per_pass || ((uintptr_t)buf_dev & 15u)) return ADSB_E_ARG;
    HIPCHK(hipSetDevice(c->cfg.device));
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0));
    HIPCHK(hipEventCreate(&e1));
    // the fastest of the read shapes (adsb_kernels.hip, read_only_kernel): none of them wins on every box and size
    double best = 0;
    for (int shape = 0; shape < adsbk::kReadShapes; ++shape) {
        HIPCHK(adsbk::launch_read_only(c->stream, buf_dev, bytes, c->scratch + 8, shape)); // warm-up
        HIPCHK(hipEventRecord(e0, c->stream));
        for (int k = 0; k < iters; ++k) HIPCHK(adsbk::launch_read_only(c->stream, buf_dev, bytes, c->scratch + 8, shape));
        HIPCHK(hipEventRecord(e1, c->stream));
        HIPCHK(hipEventSynchronize(e1));
        float ms = 0;
        HIPCHK(hipEventElapsedTime(&ms, e0, e1));
        if (shape == 0 || (double)ms / iters < best) best = (double)ms / iters;
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    *ms_per_pass = best;
    return ADSB_OK;
}

extern "C" int adsb_debug_magnitudes(adsb_ctx *c, const void *iq_host, size_t n, uint16_t *mags_host)
{
    if (!c || !iq_host || !mags_host) return ADSB_E_ARG;
    if (n == 0) return ADSB_OK;
    HIPCHK(hipSetDevice(c->cfg.device));
    void *d_in = nullptr;
    uint16_t *d_out = nullptr;
    HIPCHK(hipMalloc(&d_in, n * c->bps + 16));
    hipError_t e = hipMalloc((void **)&d_out, n * sizeof(uint16_t));
    if (e != hipSuccess) { (void)hipFree(d_in); return (int)e; }
    int rc = ADSB_OK;
    do {
        if ((e = hipMemcpyAsync(d_in, iq_host, n * c->bps, hipMemcpyHostToDevice, c->stream)) != hipSuccess) break;
        if ((e = adsbk::launch_magnitudes(c->stream, c->cfg.sample_type, c->mag_mode, d_in, n, d_out)) != hipSuccess) break;
        if ((e = hipMemcpyAsync(mags_host, d_out, n * sizeof(uint16_t), hipMemcpyDeviceToHost, c->stream)) != hipSuccess) break;
        e = hipStreamSynchronize(c->stream);
    } while (0);
    if (e != hipSuccess) rc = (int)e;
    (void)hipFree(d_in);
    (void)hipFree(d_out);
    return rc;
}

extern "C" int adsb_debug_nsq_values(adsb_ctx *c, const void *iq_host, size_t n, uint16_t *vals_host)
{
    if (!c || !iq_host || !vals_host) return ADSB_E_ARG;
    if (c->cfg.sample_type != ADSB_SAMPLE_I8) return ADSB_E_STATE;
    if (n == 0) return ADSB_OK;
    HIPCHK(hipSetDevice(c->cfg.device));
    void *d_in = nullptr;
    uint16_t *d_out = nullptr;
    HIPCHK(hipMalloc(&d_in, n * 2 + 16));
    hipError_t e = hipMalloc((void **)&d_out, n * sizeof(uint16_t));
    if (e != hipSuccess) { (void)hipFree(d_in); return (int)e; }
    do {
        if ((e = hipMemcpyAsync(d_in, iq_host, n * 2, hipMemcpyHostToDevice, c->stream)) != hipSuccess) break;
        if ((e = adsbk::launch_nsq_values(c->stream, d_in, n, d_out)) != hipSuccess) break;
        if ((e = hipMemcpyAsync(vals_host, d_out, n * sizeof(uint16_t), hipMemcpyDeviceToHost, c->stream)) != hipSuccess) break;
        e = hipStreamSynchronize(c->stream);
    } while (0);
    (void)hipFree(d_in);
    (void)hipFree(d_out);
    return e == hipSuccess ? ADSB_OK : (int)e;
}

// ---- synthetic source ------------------------------------------------------------------------------
extern "C" void adsb_synth_default(adsb_synth_cfg *s)
{
    if (!s) return;
    std::memset(s, 0, sizeof(*s));
    s->seed = 0x0AD5B0001ull;
    s->slot_len = 2000;  // one frame slot per millisecond of 2 MSPS signal
    s->frame_pct = 100;
    s->pct_flip_data = 5;
    s->pct_flip_crc = 2;
    s->pct_flip_two = 3;
    s->noise_div = 18;   // Irwin-Hall(4 bytes)/18: sigma ~ 8.2 LSB
    s->amp_shift = 0;
}

static bool synth_ok(const adsb_synth_cfg *s)
{
    return s && s->slot_len >= 256 && s->frame_pct <= 100 && s->noise_div >= 1 && s->amp_shift <= 7 &&
           s->pct_flip_data + s->pct_flip_crc + s->pct_flip_two <= 100;
}

extern "C" int adsb_synth_slot(const adsb_synth_cfg *cfg, uint32_t channel, uint64_t slot,
                               uint64_t *start, uint8_t clean14[14], uint8_t sent14[14], int *kind)
{
    if (!synth_ok(cfg)) return ADSB_E_ARG;
    adsb_synth::Slot s;
    adsb_synth::slot_params(*cfg, channel, slot, s);
    if (start) *start = slot * (uint64_t)cfg->slot_len + s.jitter;
    if (clean14) std::memcpy(clean14, s.clean, 14);
    if (sent14) std::memcpy(sent14, s.sent, 14);
    if (kind) *kind = s.kind;
    return s.present ? 1 : 0;
}

extern "C" int adsb_synth_fill_host(const adsb_synth_cfg *cfg, int sample_type, uint32_t channel,
                                    uint64_t first, size_t n, void *iq)
{
    if (!synth_ok(cfg) || (!iq && n) || (sample_type != ADSB_SAMPLE_I8 && sample_type != ADSB_SAMPLE_I16))
        return ADSB_E_ARG;
    int8_t *o8 = (int8_t *)iq;
    int16_t *o16 = (int16_t *)iq;
    uint64_t cur_slot = ~0ull;
    adsb_synth::Slot s{};
    for (size_t j = 0; j < n; ++j) {
        const uint64_t k = first + j;
        const uint64_t slot = k / cfg->slot_len;
        if (slot != cur_slot) {
            adsb_synth::slot_params(*cfg, channel, slot, s);
            cur_slot = slot;
        }
        int vi, vq;
        adsb_synth::sample_iq(*cfg, channel, k, s, slot, vi, vq);
        if (sample_type == ADSB_SAMPLE_I8) {
            o8[2 * j] = (int8_t)adsb_synth::clip8(vi);
            o8[2 * j + 1] = (int8_t)adsb_synth::clip8(vq);
        } else {
            int wi = vi << cfg->amp_shift, wq = vq << cfg->amp_shift;
            wi = wi < -32768 ? -32768 : (wi > 32767 ? 32767 : wi);
            wq = wq < -32768 ? -32768 : (wq > 32767 ? 32767 : wq);
            o16[2 * j] = (int16_t)wi;
            o16[2 * j + 1] = (int16_t)wq;
        }
    }
    return ADSB_OK;
}

extern "C" int adsb_synth_fill_device(adsb_ctx *c, const adsb_synth_cfg *cfg, uint32_t channel,
                                      uint64_t first, size_t n, void *iq_dev)
{
    if (!c || !synth_ok(cfg) || (!iq_dev && n)) return ADSB_E_ARG;
    HIPCHK(hipSetDevice(c->cfg.device));
    HIPCHK(adsbk::launch_synth(c->stream, *cfg, c->cfg.sample_type, channel, first, n, iq_dev));
    return ADSB_OK;
}

extern "C" int adsb_debug_synth_geometry(uint32_t *threads)
{
    if (threads) *threads = adsbk::synth_geometry();
    return ADSB_OK;
}
