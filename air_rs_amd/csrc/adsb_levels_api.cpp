// adsb_levels_api.cpp -- the C boundary of the levels (include/adsb_hip.h, "Per-frame signal and noise power"): argument
// checks, the grid's size, the records of a launch and of a caller's list, the copy of a host list, and the fetch.  The
// kernel is adsb_levels.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "adsb_levels.h"
#include "adsb_scratch.h"

// The levels kernel walks its frames in a grid-stride loop, one wave each: the grid is sized from the device (a few
// waves per SIMD hide the latency of the scattered 480-byte reads), not from max_out, and never above one wave per frame.
static uint32_t levels_grid(adsb_ctx *c, uint64_t cap)
{
    if (!c->levels_blocks) {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->cfg.device) != hipSuccess || cus <= 0) {
            (void)hipGetLastError();
            cus = 256;
        }
        c->levels_blocks = (uint32_t)cus * 8u; // 8 blocks of 4 waves per CU: 8 waves per SIMD
    }
    return (uint32_t)std::min<uint64_t>((cap + 3) / 4, c->levels_blocks);
}

extern "C" int adsb_levels_device_async(adsb_ctx *c)
{
    if (!c) return ADSB_E_ARG;
    if (!c->launched) return ADSB_E_STATE;
    HIPCHK(hipSetDevice(c->cfg.device));
    if (!c->levels) { // sized once, to max_out (a plain pointer: the tracker and correlate read it too)
        DevBuf<adsb_frame_level> b;
        const int rc = grow(c, b, (size_t)c->cfg.max_out);
        if (rc != ADSB_OK) return rc;
        c->levels = b.p;
    }
    adsbk::LevelsArgs a{};
    const adsb_ctx::ResultSet::Launch &li = c->launch();
    a.iq = li.iq;
    a.n_samples = li.samples;
    a.channel_stride = li.stride;
    a.offset_base = li.base;
    a.frames = li.out;
    a.hdr = c->rs[c->last].hdr;
    a.cap = li.cap;
    a.n_channels = li.channels;
    a.chan_prefix = c->rs[c->last].chan_prefix;
    a.out = c->levels;
    // same stream as the ordering pass, so it sees the finished list and header
    HIPCHK(adsbk::launch_frame_levels(c->aux, c->cfg.sample_type, a, levels_grid(c, a.cap)));
    c->levels_current = true;
    return ADSB_OK;
}

extern "C" int adsb_levels_device(adsb_ctx *c, const adsb_frame_level **levels_dev)
{
    if (!c || !levels_dev) return ADSB_E_ARG;
    *levels_dev = c->levels;
    return c->levels ? ADSB_OK : ADSB_E_STATE;
}

extern "C" int adsb_fetch_levels(adsb_ctx *c, adsb_frame_level *out, size_t max_out, size_t *n_out)
{
    if (!c || !n_out || (!out && max_out)) return ADSB_E_ARG;
    if (!c->launched || !c->levels || !c->levels_current) return ADSB_E_STATE;
    int rc = sync_header(c);
    if (rc != ADSB_OK) return rc;
    // the wait found holes in the list and rebuilt it (slot-pool overflow): the levels enqueued before are of the list
    // with holes.  Again, for the rebuilt one (the host has waited for the rebuild).
    if (!c->levels_current && (rc = adsb_levels_device_async(c)) != ADSB_OK) return rc;
    uint64_t n = std::min<uint64_t>(c->hdr_host->n_out, c->launch().cap);
    if (n > max_out) n = max_out;
    if (n) HIPCHK(hipMemcpyAsync(out, c->levels, sizeof(adsb_frame_level) * n, hipMemcpyDeviceToHost, c->aux));
    HIPCHK(hipStreamSynchronize(c->aux));
    *n_out = (size_t)n;
    return ADSB_OK;
}

extern "C" int adsb_levels_of(adsb_ctx *c, const void *iq_dev, size_t n_samples, uint64_t first_sample_index,
                              const adsb_frame *frames, size_t n, adsb_frame_level *out)
{
    if (!c || !iq_dev || ((!frames || !out) && n)) return ADSB_E_ARG;
    if ((uintptr_t)iq_dev & (c->bps - 1u)) return ADSB_E_ARG;
    if (n > 0xFFFFFFFFull) return ADSB_E_CAPACITY;
    if (n == 0) return ADSB_OK;
    HIPCHK(hipSetDevice(c->cfg.device));
    int rc = grow(c, c->lvof_out, n);
    if (rc != ADSB_OK) return rc;
    const adsb_frame *list = nullptr;
    if ((rc = stage_list(c, frames, n, c->lvof_frames, &list)) != ADSB_OK) return rc;
    adsbk::LevelsArgs a{};
    a.iq = iq_dev;
    a.n_samples = n_samples;
    a.channel_stride = n_samples;
    a.offset_base = first_sample_index;
    a.frames = list;
    a.hdr = nullptr;
    a.cap = (uint32_t)n;
    a.n_channels = 1;
    a.chan_prefix = nullptr;
    a.out = c->lvof_out.p;
    HIPCHK(adsbk::launch_frame_levels(c->aux, c->cfg.sample_type, a, levels_grid(c, n)));
    HIPCHK(hipMemcpyAsync(out, c->lvof_out.p, sizeof(adsb_frame_level) * n, hipMemcpyDeviceToHost, c->aux));
    HIPCHK(hipStreamSynchronize(c->aux)); // (nothing uses the scratch any more: the next call may grow it without a wait)
    return ADSB_OK;
}

extern "C" int adsb_levels_modes_of(adsb_ctx *c, const void *iq_dev, uint32_t n_channels, size_t n_samples,
                                    size_t channel_stride, uint64_t first_sample_index, const adsb_frame *frames,
                                    const uint64_t *counts, size_t n, adsb_frame_level *out)
{
    if (!c) return ADSB_E_ARG;
    int rc = adsbk::levels_modes_args_check(iq_dev, n_channels, n_samples, channel_stride, frames, counts, n);
    if (rc != ADSB_OK) return rc;
    if ((uintptr_t)iq_dev & (c->bps - 1u)) return ADSB_E_ARG;
    if (n == 0) return ADSB_OK; // nothing allocated, nothing launched; an earlier call's records stay
    HIPCHK(hipSetDevice(c->cfg.device));
    c->lvm_done = false; // until the records are complete: a call that fails on the way leaves none
    if ((rc = grow(c, c->lvm_out, n)) != ADSB_OK) return rc;
    const adsb_frame *list = nullptr;
    if ((rc = stage_list(c, frames, n, c->lvm_frames, &list)) != ADSB_OK) return rc;
    std::vector<uint64_t> prefix((size_t)n_channels + 1, 0);
    for (uint32_t ch = 0; ch < n_channels; ++ch) prefix[ch + 1] = prefix[ch] + counts[ch];
    if (n_channels > 1) {
        if ((rc = grow(c, c->lvm_prefix, prefix.size())) != ADSB_OK) return rc;
        HIPCHK(hipMemcpyAsync(c->lvm_prefix.p, prefix.data(), 8 * prefix.size(), hipMemcpyHostToDevice, c->aux));
    }
    adsbk::LevelsModesArgs a{};
    a.iq = iq_dev;
    a.n_samples = n_samples;
    a.channel_stride = n_channels == 1 ? n_samples : channel_stride;
    a.offset_base = first_sample_index;
    a.frames = list;
    a.n = (uint32_t)n;
    a.n_channels = n_channels;
    a.prefix = n_channels > 1 ? c->lvm_prefix.p : nullptr;
    a.out = c->lvm_out.p;
    HIPCHK(adsbk::launch_frame_levels_modes(c->aux, c->cfg.sample_type, a, levels_grid(c, n)));
    if (out) HIPCHK(hipMemcpyAsync(out, c->lvm_out.p, sizeof(adsb_frame_level) * n, hipMemcpyDeviceToHost, c->aux));
    HIPCHK(hipStreamSynchronize(c->aux)); // the host list and the prefix are the caller's again; the records are complete
    c->lvm_done = true;
    return ADSB_OK;
}

extern "C" int adsb_levels_modes_device(adsb_ctx *c, const adsb_frame_level **levels_dev)
{
    if (!c || !levels_dev) return ADSB_E_ARG;
    *levels_dev = c->lvm_done ? c->lvm_out.p : nullptr;
    return c->lvm_done ? ADSB_OK : ADSB_E_STATE;
}
