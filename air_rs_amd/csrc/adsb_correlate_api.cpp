// adsb_correlate_api.cpp -- the C boundary of correlate (include/adsb_hip.h, "Correlate"): argument checks, the one
// device block the kernels' arrays are carved from, the copies of host lists, and the fetch.  The kernels are
// adsb_correlate.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "adsb_correlate.h"
#include "adsb_ctx.h"

static bool corr_in_device_memory(const adsb_ctx *c, const void *p)
{
    hipPointerAttribute_t at{};
    const bool yes = hipPointerGetAttributes(&at, p) == hipSuccess && at.type == hipMemoryTypeDevice &&
                     at.device == c->cfg.device;
    (void)hipGetLastError(); // a plain host pointer is an error to the query: do not leave it to the launches after it
    return yes;
}

// One block for `frames` receptions (at least one).  Every array starts 256-byte aligned.
static int corr_reserve(adsb_ctx *c, size_t frames)
{
    adsb_ctx::Corr &k = c->corr;
    if (k.block && k.frames >= frames) return ADSB_OK;
    if (k.block) HIPCHK(hipStreamSynchronize(c->aux)); // an earlier call's kernels may still use the block
    (void)hipFree(k.block);
    k = adsb_ctx::Corr{};
    const size_t f = std::max<size_t>(frames, 1);
    const size_t temp_bytes = adsbk::corr_temp_bytes(f);
    if (temp_bytes == 0) return ADSB_E_NOMEM;
    size_t total = 0;
    const auto take = [&total](size_t bytes) {
        const size_t at = total;
        total += (bytes + 255) & ~(size_t)255;
        return at;
    };
    const size_t o_t = take(8 * f), o_lo = take(8 * f), o_hi = take(8 * f), o_ht = take(8 * f);
    const size_t o_rx = take(4 * f), o_ord = take(4 * f), o_pos = take(4 * f), o_midx = take(4 * f);
    const size_t o_scan = take(sizeof(adsbk::CorrAgg) * f), o_temp = take(temp_bytes);
    const size_t o_msgs = take(sizeof(adsb_message) * f), o_fout = take(sizeof(adsb_frame) * f);
    const size_t o_recs = take(sizeof(adsb_reception) * f), o_hdr = take(2 * sizeof(uint64_t));
    const size_t o_prefix = take(8 * (adsbk::kCorrMaxReceivers + 1)), o_base = take(8 * adsbk::kCorrMaxReceivers);
    const size_t o_inf = take(sizeof(adsb_frame) * f), o_inl = take(sizeof(adsb_frame_level) * f);
    char *b = nullptr;
    if (hipMalloc((void **)&b, total) != hipSuccess) {
        (void)hipGetLastError();
        return ADSB_E_NOMEM;
    }
    k.block = b;
    k.frames = f;
    adsbk::CorrArgs &a = k.a;
    a.t = (uint64_t *)(b + o_t);
    a.lo = (uint64_t *)(b + o_lo);
    a.hi = (uint64_t *)(b + o_hi);
    a.head_t = (uint64_t *)(b + o_ht);
    a.rx = (uint32_t *)(b + o_rx);
    a.ord = (uint32_t *)(b + o_ord);
    a.pos = (uint32_t *)(b + o_pos);
    a.midx = (uint32_t *)(b + o_midx);
    a.scan = (adsbk::CorrAgg *)(b + o_scan);
    a.temp = b + o_temp;
    a.temp_bytes = temp_bytes;
    a.msgs = (adsb_message *)(b + o_msgs);
    a.frames_out = (adsb_frame *)(b + o_fout);
    a.recs = (adsb_reception *)(b + o_recs);
    a.hdr = (uint64_t *)(b + o_hdr);
    k.prefix = (uint64_t *)(b + o_prefix);
    k.base = (uint64_t *)(b + o_base);
    k.in_frames = (adsb_frame *)(b + o_inf);
    k.in_levels = (adsb_frame_level *)(b + o_inl);
    return ADSB_OK;
}

// prefix[n_receivers + 1] (host, last = n): the checked split of an n-frame list.  Enqueues on c->aux and returns once the
// host arrays are copied; the kernels run behind.
static int corr_run(adsb_ctx *c, const adsb_correlate_cfg &cfg, const adsb_frame *frames, const adsb_frame_level *levels,
                    size_t n, const uint64_t *prefix, uint32_t n_receivers, const uint64_t *sample_base, size_t reserve)
{
    int rc = corr_reserve(c, std::max(reserve, n));
    if (rc != ADSB_OK) return rc;
    adsb_ctx::Corr &k = c->corr;
    adsbk::CorrArgs a = k.a;
    a.n = (uint32_t)n;
    a.n_receivers = n_receivers;
    a.window = cfg.window;
    a.frames = frames;
    a.levels = levels;
    a.prefix = k.prefix;
    a.base = sample_base ? k.base : nullptr;
    if (n) {
        if (!corr_in_device_memory(c, frames)) {
            HIPCHK(hipMemcpyAsync(k.in_frames, frames, sizeof(adsb_frame) * n, hipMemcpyHostToDevice, c->aux));
            a.frames = k.in_frames;
        }
        if (levels && !corr_in_device_memory(c, levels)) {
            HIPCHK(hipMemcpyAsync(k.in_levels, levels, sizeof(adsb_frame_level) * n, hipMemcpyHostToDevice, c->aux));
            a.levels = k.in_levels;
        }
        HIPCHK(hipMemcpyAsync(k.prefix, prefix, sizeof(uint64_t) * ((size_t)n_receivers + 1), hipMemcpyHostToDevice, c->aux));
        if (sample_base)
            HIPCHK(hipMemcpyAsync(k.base, sample_base, sizeof(uint64_t) * n_receivers, hipMemcpyHostToDevice, c->aux));
        HIPCHK(hipStreamSynchronize(c->aux)); // the host arrays are the caller's (and this frame's) again
    }
    HIPCHK(adsbk::launch_correlate(c->aux, a));
    k.done = true;
    k.n = a.n;
    return ADSB_OK;
}

extern "C" int adsb_correlate_of(adsb_ctx *c, const adsb_correlate_cfg *cfg, const adsb_frame *frames,
                                 const adsb_frame_level *levels, size_t n, const uint64_t *counts, uint32_t n_receivers,
                                 const uint64_t *sample_base)
{
    if (!c || !cfg || !counts || n_receivers < 1 || n_receivers > adsbk::kCorrMaxReceivers || (!frames && n))
        return ADSB_E_ARG;
    if ((uint64_t)n > 0xFFFFFFFFull) return ADSB_E_CAPACITY;
    std::vector<uint64_t> prefix((size_t)n_receivers + 1, 0);
    for (uint32_t r = 0; r < n_receivers; ++r) {
        if (counts[r] > (uint64_t)n - prefix[r]) return ADSB_E_ARG;
        prefix[r + 1] = prefix[r] + counts[r];
    }
    if (prefix[n_receivers] != (uint64_t)n) return ADSB_E_ARG;
    HIPCHK(hipSetDevice(c->cfg.device));
    return corr_run(c, *cfg, frames, levels, n, prefix.data(), n_receivers, sample_base, 0);
}

extern "C" int adsb_correlate_launch(adsb_ctx *c, const adsb_correlate_cfg *cfg, const uint64_t *sample_base)
{
    if (!c || !cfg) return ADSB_E_ARG;
    if (!c->launched) return ADSB_E_STATE;
    if (c->last_channels > adsbk::kCorrMaxReceivers) return ADSB_E_ARG;
    int rc = sync_header(c); // the list's length, as adsb_fetch_counts (and the rebuild after a slot-pool overflow)
    if (rc != ADSB_OK) return rc;
    const uint64_t n = std::min<uint64_t>(c->hdr_host->n_out, c->last_cap);
    HIPCHK(hipSetDevice(c->cfg.device));
    // not enqueued yet for this launch, or of the list with holes that sync_header has just rebuilt: (again) now, on the
    // stream the correlate kernels follow on
    const bool with_levels = cfg->use_levels != 0;
    if (with_levels && n && !(c->levels && c->levels_current) && (rc = adsb_levels_device_async(c)) != ADSB_OK) return rc;
    adsb_ctx::ResultSet &r = c->rs[c->last];
    // the channel split as adsb_fetch's per_channel_counts reads it: chan_prefix clipped to the list
    std::vector<uint64_t> prefix((size_t)c->last_channels + 1);
    HIPCHK(hipMemcpyAsync(prefix.data(), r.chan_prefix, sizeof(uint64_t) * prefix.size(), hipMemcpyDeviceToHost, c->aux));
    HIPCHK(hipStreamSynchronize(c->aux));
    for (uint64_t &p : prefix) p = std::min<uint64_t>(p, n);
    prefix[0] = 0;
    prefix[c->last_channels] = n;
    if ((rc = corr_run(c, *cfg, c->last_out, with_levels && n ? c->levels : nullptr, (size_t)n, prefix.data(),
                       c->last_channels, sample_base, (size_t)c->cfg.max_out)) != ADSB_OK)
        return rc;
    if (c->own_aux) { // the launch that reuses this result set waits for these kernels too
        HIPCHK(hipEventRecord(r.g_done, c->aux));
        r.g_pending = true;
    }
    return ADSB_OK;
}

extern "C" int adsb_fetch_correlated(adsb_ctx *c, adsb_message *msgs, size_t max_msgs, size_t *n_msgs, adsb_reception *recs,
                                     size_t max_recs, size_t *n_recs)
{
    if (!c || (!msgs && max_msgs) || (!recs && max_recs)) return ADSB_E_ARG;
    const adsb_ctx::Corr &k = c->corr;
    if (!k.done) return ADSB_E_STATE;
    HIPCHK(hipSetDevice(c->cfg.device));
    uint64_t hdr[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(hdr, k.a.hdr, sizeof(hdr), hipMemcpyDeviceToHost, c->aux));
    HIPCHK(hipStreamSynchronize(c->aux));
    const size_t nm = std::min<size_t>((size_t)hdr[0], max_msgs), nr = std::min<size_t>((size_t)hdr[1], max_recs);
    if (nm) HIPCHK(hipMemcpyAsync(msgs, k.a.msgs, sizeof(adsb_message) * nm, hipMemcpyDeviceToHost, c->aux));
    if (nr) HIPCHK(hipMemcpyAsync(recs, k.a.recs, sizeof(adsb_reception) * nr, hipMemcpyDeviceToHost, c->aux));
    HIPCHK(hipStreamSynchronize(c->aux));
    if (n_msgs) *n_msgs = (size_t)hdr[0];
    if (n_recs) *n_recs = (size_t)hdr[1];
    return ADSB_OK;
}

extern "C" int adsb_correlated_device(adsb_ctx *c, const adsb_message **msgs_dev, const adsb_frame **frames_dev,
                                      const adsb_reception **recs_dev, const void **header_dev)
{
    if (!c) return ADSB_E_ARG;
    const adsb_ctx::Corr &k = c->corr;
    if (!k.done) return ADSB_E_STATE;
    if (msgs_dev) *msgs_dev = k.a.msgs;
    if (frames_dev) *frames_dev = k.a.frames_out;
    if (recs_dev) *recs_dev = k.a.recs;
    if (header_dev) *header_dev = k.a.hdr;
    return ADSB_OK;
}

extern "C" int adsb_debug_correlate_geometry(uint32_t *threads_per_block)
{
    if (threads_per_block) *threads_per_block = adsbk::kCorrBlock;
    return ADSB_OK;
}
