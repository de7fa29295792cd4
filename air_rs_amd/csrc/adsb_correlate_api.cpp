// adsb_correlate_api.cpp -- the C boundary of correlate (include/adsb_hip.h, "Correlate"): argument checks, the one
// device block the kernels' arrays are carved from, the copies of host lists, and the fetch.  The kernels are
// adsb_correlate.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "adsb_correlate.h"
#include "adsb_scratch.h"

// One block for `frames` receptions (at least one).  Every array starts 256-byte aligned.
static int corr_reserve(adsb_ctx *c, size_t frames)
{
    adsb_ctx::Corr &k = c->corr;
    if (k.mem.p && k.frames >= frames) return ADSB_OK;
    const size_t f = std::max<size_t>(frames, 1);
    const size_t temp_bytes = adsbk::corr_temp_bytes(f);
    k.done = false;
    k.frames = 0;
    if (temp_bytes == 0) return ADSB_E_NOMEM;
    const int rc = carve_block(c, k.mem, [&k, f, temp_bytes](Carve &cv) {
        adsbk::CorrArgs &a = k.a;
        a.t = cv.take<uint64_t>(f);
        a.lo = cv.take<uint64_t>(f);
        a.hi = cv.take<uint64_t>(f);
        a.head_t = cv.take<uint64_t>(f);
        a.rx = cv.take<uint32_t>(f);
        a.ord = cv.take<uint32_t>(f);
        a.pos = cv.take<uint32_t>(f);
        a.midx = cv.take<uint32_t>(f);
        a.scan = cv.take<adsbk::CorrAgg>(f);
        a.temp = cv.take<char>(temp_bytes);
        a.temp_bytes = temp_bytes;
        a.msgs = cv.take<adsb_message>(f);
        a.frames_out = cv.take<adsb_frame>(f);
        a.recs = cv.take<adsb_reception>(f);
        a.hdr = cv.take<uint64_t>(2);
        k.prefix = cv.take<uint64_t>(adsbk::kCorrMaxReceivers + 1);
        k.base = cv.take<uint64_t>(adsbk::kCorrMaxReceivers);
        k.in_frames = cv.take<adsb_frame>(f);
        k.in_levels = cv.take<adsb_frame_level>(f);
    });
    if (rc != ADSB_OK) return rc;
    k.frames = f;
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
        if (!in_device_memory(c, frames)) {
            HIPCHK(hipMemcpyAsync(k.in_frames, frames, sizeof(adsb_frame) * n, hipMemcpyHostToDevice, c->aux));
            a.frames = k.in_frames;
        }
        if (levels && !in_device_memory(c, levels)) {
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
    if (c->launch().channels > adsbk::kCorrMaxReceivers) return ADSB_E_ARG;
    int rc = sync_header(c); // the list's length, as adsb_fetch_counts (and the rebuild after a slot-pool overflow)
    if (rc != ADSB_OK) return rc;
    const uint64_t n = std::min<uint64_t>(c->hdr_host->n_out, c->launch().cap);
    HIPCHK(hipSetDevice(c->cfg.device));
    // not enqueued yet for this launch, or of the list with holes that sync_header has just rebuilt: (again) now, on the
    // stream the correlate kernels follow on
    const bool with_levels = cfg->use_levels != 0;
    if (with_levels && n && !(c->levels && c->levels_current) && (rc = adsb_levels_device_async(c)) != ADSB_OK) return rc;
    adsb_ctx::ResultSet &r = c->rs[c->last];
    // the channel split as adsb_fetch's per_channel_counts reads it: chan_prefix clipped to the list
    std::vector<uint64_t> prefix((size_t)c->launch().channels + 1);
    HIPCHK(hipMemcpyAsync(prefix.data(), r.chan_prefix, sizeof(uint64_t) * prefix.size(), hipMemcpyDeviceToHost, c->aux));
    HIPCHK(hipStreamSynchronize(c->aux));
    for (uint64_t &p : prefix) p = std::min<uint64_t>(p, n);
    prefix[0] = 0;
    prefix[c->launch().channels] = n;
    if ((rc = corr_run(c, *cfg, c->launch().out, with_levels && n ? c->levels : nullptr, (size_t)n, prefix.data(),
                       c->launch().channels, sample_base, (size_t)c->cfg.max_out)) != ADSB_OK)
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
