// adsb_wire_api.cpp -- the C boundary of the wire output (include/adsb_hip.h, "Wire output"): argument checks, the one
// device block the stream and its ends are carved from, the copies of host lists, and the fetch.  The kernels are
// adsb_wire.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "adsb_scratch.h"
#include "adsb_wire.h"

// One block for the stream of `frames` frames (at least one).  Every array starts 256-byte aligned.
static int wire_reserve(adsb_ctx *c, adsb_ctx::Wire *w, size_t frames)
{
    if (frames * (uint64_t)adsbk::kWireMaxBytes > 0xFFFFFFFFull) return ADSB_E_CAPACITY; // ends[] are 32 bits wide
    if (w->frames >= frames && w->hdr) return ADSB_OK;
    const size_t f = std::max<size_t>(frames, 1);
    const int rc = carve_block(c, w->mem, [w, f](Carve &cv) {
        w->out = cv.take<uint8_t>(f * adsbk::kWireMaxBytes);
        w->ends = cv.take<uint32_t>(f);
        w->block = cv.take<uint32_t>(adsbk::wire_blocks(f));
        w->hdr = cv.take<uint64_t>(2);
    });
    if (rc != ADSB_OK) {
        *w = adsb_ctx::Wire{}; // (a non-null hdr says "allocated")
        return rc;
    }
    w->frames = frames;
    return ADSB_OK;
}

static adsbk::WireArgs wire_args(const adsb_ctx *c, const adsb_ctx::Wire &w, const adsb_wire_cfg &cfg)
{
    adsbk::WireArgs a{};
    a.format = cfg.format;
    a.sample_type = c->cfg.sample_type;
    a.tick_bias = cfg.tick_bias;
    a.out = w.out;
    a.ends = w.ends;
    a.block = w.block;
    a.wire_hdr = w.hdr;
    return a;
}

static bool wire_wants_levels(const adsb_wire_cfg &cfg) { return cfg.signal != 0 && adsbk::wire_base_format(cfg.format) == ADSB_WIRE_BEAST; }

extern "C" int adsb_wire_device_async(adsb_ctx *c, const adsb_wire_cfg *cfg)
{
    if (!c || !adsbk::wire_cfg_ok(cfg)) return ADSB_E_ARG;
    if (!c->launched) return ADSB_E_STATE;
    HIPCHK(hipSetDevice(c->cfg.device));
    int rc = wire_reserve(c, &c->wire, (size_t)c->cfg.max_out);
    if (rc != ADSB_OK) return rc;
    if (wire_wants_levels(*cfg) && !c->levels_current && (rc = adsb_levels_device_async(c)) != ADSB_OK) return rc;
    adsbk::WireArgs a = wire_args(c, c->wire, *cfg);
    a.frames = c->launch().out;
    a.levels = wire_wants_levels(*cfg) ? c->levels : nullptr;
    a.hdr = c->rs[c->last].hdr;
    a.cap = c->launch().cap;
    // same stream as the ordering pass (and the levels kernel), so it sees the finished list, header and levels
    HIPCHK(adsbk::launch_wire(c->aux, a));
    c->wire_cfg = *cfg;
    c->wire_current = true;
    return ADSB_OK;
}

extern "C" int adsb_wire_device(adsb_ctx *c, const uint8_t **bytes_dev, const uint32_t **ends_dev, const void **header_dev)
{
    if (!c) return ADSB_E_ARG;
    if (bytes_dev) *bytes_dev = c->wire.out;
    if (ends_dev) *ends_dev = c->wire.ends;
    if (header_dev) *header_dev = c->wire.hdr;
    return c->wire.hdr ? ADSB_OK : ADSB_E_STATE;
}

// The finished stream of `w` (n frames encoded on c->aux) to the host: the whole of it if cap holds it, else the longest
// prefix of whole frames; ends[] takes min(n, max_ends) entries.
static int wire_copy_out(adsb_ctx *c, const adsb_ctx::Wire &w, uint8_t *out, size_t cap, size_t *n_bytes, uint32_t *ends,
                         size_t max_ends, size_t *n_frames)
{
    uint64_t hdr[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(hdr, w.hdr, sizeof(hdr), hipMemcpyDeviceToHost, c->aux));
    HIPCHK(hipStreamSynchronize(c->aux));
    const size_t total = (size_t)hdr[0], n = (size_t)hdr[1];
    size_t take = total;
    std::vector<uint32_t> all;
    const uint32_t *host_ends = nullptr;
    const size_t n_ends = ends ? std::min(n, max_ends) : 0;
    if (total > cap) { // whole frames only: the last end at or below cap
        all.resize(n);
        HIPCHK(hipMemcpyAsync(all.data(), w.ends, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, c->aux));
        HIPCHK(hipStreamSynchronize(c->aux));
        const size_t k = (size_t)(std::upper_bound(all.begin(), all.end(), (uint32_t)std::min<size_t>(cap, 0xFFFFFFFFu)) - all.begin());
        take = k ? all[k - 1] : 0;
        host_ends = all.data();
    }
    if (take) HIPCHK(hipMemcpyAsync(out, w.out, take, hipMemcpyDeviceToHost, c->aux));
    if (n_ends) {
        if (host_ends) std::memcpy(ends, host_ends, sizeof(uint32_t) * n_ends);
        else HIPCHK(hipMemcpyAsync(ends, w.ends, sizeof(uint32_t) * n_ends, hipMemcpyDeviceToHost, c->aux));
    }
    HIPCHK(hipStreamSynchronize(c->aux));
    *n_bytes = total;
    if (n_frames) *n_frames = n;
    return ADSB_OK;
}

extern "C" int adsb_fetch_wire(adsb_ctx *c, uint8_t *out, size_t cap, size_t *n_bytes, uint32_t *ends, size_t max_ends,
                               size_t *n_frames)
{
    if (!c || !n_bytes || !n_frames || (!out && cap) || (!ends && max_ends)) return ADSB_E_ARG;
    if (!c->launched || !c->wire.hdr || !c->wire_current) return ADSB_E_STATE;
    int rc = sync_header(c);
    if (rc != ADSB_OK) return rc;
    // the wait found holes in the list and rebuilt it (slot-pool overflow): the stream enqueued before is of the list
    // with holes.  Again, for the rebuilt one (and its levels, which the same wait marked stale).
    if (!c->wire_current) {
        const adsb_wire_cfg cfg = c->wire_cfg;
        if ((rc = adsb_wire_device_async(c, &cfg)) != ADSB_OK) return rc;
    }
    return wire_copy_out(c, c->wire, out, cap, n_bytes, ends, max_ends, n_frames);
}

extern "C" int adsb_wire_of(adsb_ctx *c, const adsb_wire_cfg *cfg, const adsb_frame *frames, const adsb_frame_level *levels,
                            size_t n, uint8_t *out, size_t cap, size_t *n_bytes, uint32_t *ends)
{
    if (!c || !adsbk::wire_cfg_ok(cfg) || !n_bytes || (!frames && n) || (!out && cap)) return ADSB_E_ARG;
    if (n * (uint64_t)adsbk::kWireMaxBytes > 0xFFFFFFFFull) return ADSB_E_CAPACITY;
    HIPCHK(hipSetDevice(c->cfg.device));
    int rc = wire_reserve(c, &c->wof, n);
    if (rc != ADSB_OK) return rc;
    const adsb_frame *list = nullptr;
    const adsb_frame_level *lv = nullptr;
    if ((rc = stage_list(c, frames, n, c->wof_frames, &list)) != ADSB_OK) return rc;
    if ((rc = stage_list(c, wire_wants_levels(*cfg) ? levels : nullptr, n, c->wof_levels, &lv)) != ADSB_OK) return rc;
    adsbk::WireArgs a = wire_args(c, c->wof, *cfg);
    a.frames = list;
    a.levels = lv;
    a.hdr = nullptr;
    a.cap = (uint32_t)n;
    HIPCHK(adsbk::launch_wire(c->aux, a));
    return wire_copy_out(c, c->wof, out, cap, n_bytes, ends, n, nullptr); // (waits: nothing uses the scratch any more)
}

extern "C" int adsb_debug_wire_geometry(uint32_t *frames_per_block, uint32_t *scan_threads)
{
    if (frames_per_block) *frames_per_block = adsbk::kWireBlockFrames;
    if (scan_threads) *scan_threads = adsbk::kWireScanThreads;
    return ADSB_OK;
}
