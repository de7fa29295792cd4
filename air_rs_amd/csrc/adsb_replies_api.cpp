// adsb_replies_api.cpp -- the C boundary of the replies scan and the list merge (include/adsb_hip.h, "Mode S replies from
// samples"): argument checks, the one device block the kernels' arrays are carved from, the copies of host lists, and the
// fetch.  The kernels are adsb_replies.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "adsb_replies.h"
#include "adsb_scratch.h"

// One block for `tiles` tiles, `cap` frames and `channels` channels.  Every array starts 256-byte aligned.
static int replies_reserve(adsb_ctx *c, size_t tiles, size_t cap, size_t channels)
{
    adsb_ctx::Replies &k = c->replies;
    if (k.mem.p && k.tiles >= tiles && k.cap >= cap && k.channels >= channels) return ADSB_OK;
    tiles = std::max(tiles, k.tiles), cap = std::max(cap, k.cap), channels = std::max(channels, k.channels);
    const size_t f = std::max<size_t>(cap, 1);
    k.done = false;
    k.tiles = k.cap = k.channels = 0;
    const int rc = carve_block(c, k.mem, [&k, tiles, f, channels](Carve &cv) {
        adsbk::RepliesArgs &a = k.a;
        a = adsbk::RepliesArgs{};
        a.tile = cv.take<uint32_t>(adsbk::kRepliesTileWords * tiles);
        a.bitmap = cv.take<uint32_t>(adsbk::kRepliesThreads * tiles);
        a.group = cv.take<uint32_t>(adsbk::kRepliesTileWords * (size_t)adsbk::replies_groups(tiles));
        a.prefix = cv.take<uint64_t>(tiles + 1);
        a.frames = cv.take<adsb_frame>(f);
        a.counts = cv.take<uint64_t>(channels);
        a.hdr = cv.take<adsb_replies_header>(1);
    });
    if (rc != ADSB_OK) return rc;
    k.tiles = tiles, k.cap = cap, k.channels = channels;
    return ADSB_OK;
}

extern "C" int adsb_replies_of(adsb_ctx *c, const adsb_replies_cfg *cfg, const void *iq_dev, uint32_t n_channels,
                               size_t n_samples, size_t channel_stride, const uint32_t *known, size_t n_known)
{
    if (!c) return ADSB_E_ARG;
    HIPCHK(hipSetDevice(c->cfg.device));
    const bool known_host = n_known && known && !in_device_memory(c, known);
    int rc = adsbk::replies_args_check(cfg, iq_dev, n_channels, n_samples, channel_stride, known, n_known, known_host);
    if (rc != ADSB_OK) return rc;
    if (((uintptr_t)iq_dev & 15u) != 0 || (n_channels > 1 && (channel_stride & 7u) != 0)) return ADSB_E_ARG;
    if (n_channels > c->cfg.max_channels || n_samples > c->cfg.max_samples) return ADSB_E_CAPACITY;
    if (n_channels == 1) channel_stride = n_samples;
    const uint64_t cap = cfg->max_frames ? cfg->max_frames : c->cfg.max_out;
    const uint64_t tpc = adsbk::replies_tiles_per_channel(n_samples, adsbk::replies_tile(c->cfg.sample_type));
    if (cap > 0xFFFFFFFFull || tpc * n_channels > 0x7FFFFFFFull) return ADSB_E_CAPACITY;
    adsb_ctx::Replies &k = c->replies;
    const uint32_t *k_use = nullptr;
    if ((rc = stage_list(c, known, n_known, k.in_known, &k_use)) != ADSB_OK) return rc;
    if ((rc = replies_reserve(c, (size_t)(tpc * n_channels), (size_t)cap, n_channels)) != ADSB_OK) return rc;
    adsbk::RepliesArgs a = k.a;
    a.iq = iq_dev;
    a.n_samples = n_samples;
    a.channel_stride = channel_stride;
    a.offset_base = cfg->first_sample_index;
    a.n_channels = n_channels;
    a.tiles_per_channel = (uint32_t)tpc;
    a.n_tiles = (uint32_t)(tpc * n_channels);
    a.flags = cfg->flags;
    a.known = k_use;
    a.n_known = (uint32_t)n_known;
    a.cap = (uint32_t)cap;
    if (k_use != known) HIPCHK(hipStreamSynchronize(c->aux)); // a host list was copied: it is the caller's again
    HIPCHK(adsbk::launch_replies(c->aux, c->cfg.sample_type, a));
    k.n_channels = n_channels;
    k.done = true;
    return ADSB_OK;
}

extern "C" int adsb_fetch_replies(adsb_ctx *c, adsb_frame *out, size_t max_out, size_t *n_out, uint64_t *counts,
                                  adsb_replies_header *header)
{
    if (!c || (!out && max_out)) return ADSB_E_ARG;
    const adsb_ctx::Replies &k = c->replies;
    if (!k.done) return ADSB_E_STATE;
    HIPCHK(hipSetDevice(c->cfg.device));
    adsb_replies_header h{};
    HIPCHK(hipMemcpyAsync(&h, k.a.hdr, sizeof(h), hipMemcpyDeviceToHost, c->aux));
    HIPCHK(hipStreamSynchronize(c->aux));
    const size_t n = std::min<size_t>((size_t)h.n_out, max_out);
    if (n) HIPCHK(hipMemcpyAsync(out, k.a.frames, sizeof(adsb_frame) * n, hipMemcpyDeviceToHost, c->aux));
    if (counts) HIPCHK(hipMemcpyAsync(counts, k.a.counts, 8 * (size_t)k.n_channels, hipMemcpyDeviceToHost, c->aux));
    HIPCHK(hipStreamSynchronize(c->aux));
    if (n_out) *n_out = n;
    if (header) *header = h;
    return ADSB_OK;
}

extern "C" int adsb_replies_device(adsb_ctx *c, const adsb_frame **frames_dev, const uint64_t **counts_dev,
                                   const void **header_dev)
{
    if (!c) return ADSB_E_ARG;
    const adsb_ctx::Replies &k = c->replies;
    if (!k.done) return ADSB_E_STATE;
    if (frames_dev) *frames_dev = k.a.frames;
    if (counts_dev) *counts_dev = k.a.counts;
    if (header_dev) *header_dev = k.a.hdr;
    return ADSB_OK;
}

extern "C" int adsb_debug_replies_geometry(uint32_t *tile_offsets_i8, uint32_t *tile_offsets_i16)
{
    if (tile_offsets_i8) *tile_offsets_i8 = adsbk::replies_tile(ADSB_SAMPLE_I8);
    if (tile_offsets_i16) *tile_offsets_i16 = adsbk::replies_tile(ADSB_SAMPLE_I16);
    return ADSB_OK;
}

// n records of src, host or device memory, into dst (host memory), waiting for them
template <class T>
static int to_host(adsb_ctx *c, T *dst, const T *src, size_t n)
{
    if (!n) return ADSB_OK;
    if (in_device_memory(c, src)) {
        HIPCHK(hipMemcpyAsync(dst, src, sizeof(T) * n, hipMemcpyDeviceToHost, c->aux));
        HIPCHK(hipStreamSynchronize(c->aux));
    } else {
        std::copy(src, src + n, dst);
    }
    return ADSB_OK;
}

// *use = where the kernel writes n records bound for dst: dst itself if it is device memory, else b grown to hold them
template <class T>
static int stage_result(adsb_ctx *c, T *dst, size_t n, DevBuf<T> &b, T **use)
{
    *use = dst;
    if (!dst || !n || in_device_memory(c, dst)) return ADSB_OK;
    const int rc = grow(c, b, n);
    if (rc != ADSB_OK) return rc;
    *use = b.p;
    return ADSB_OK;
}

extern "C" int adsb_merge_lists_of(adsb_ctx *c, const adsb_frame *a, const uint64_t *counts_a, const adsb_frame *b,
                                   const uint64_t *counts_b, uint32_t n_channels, adsb_frame *out, uint32_t *src,
                                   uint64_t *counts_out)
{
    if (!c) return ADSB_E_ARG;
    HIPCHK(hipSetDevice(c->cfg.device));
    int rc = adsbk::merge_args_check(a, counts_a, b, counts_b, n_channels);
    if (rc != ADSB_OK) return rc;
    const size_t nc = n_channels;
    std::vector<uint64_t> ca(nc), cb(nc), prefix(2 * (nc + 1), 0);
    if ((rc = to_host(c, ca.data(), counts_a, nc)) != ADSB_OK) return rc;
    if ((rc = to_host(c, cb.data(), counts_b, nc)) != ADSB_OK) return rc;
    uint64_t *pa = prefix.data(), *pb = pa + nc + 1;
    for (size_t i = 0; i < nc; ++i) {
        if (ca[i] >= ADSB_MERGE_FROM_B || cb[i] >= ADSB_MERGE_FROM_B) return ADSB_E_CAPACITY;
        pa[i + 1] = pa[i] + ca[i], pb[i + 1] = pb[i] + cb[i];
        if (pa[i + 1] >= ADSB_MERGE_FROM_B || pb[i + 1] >= ADSB_MERGE_FROM_B) return ADSB_E_CAPACITY;
    }
    const size_t na = (size_t)pa[nc], nb = (size_t)pb[nc], n = na + nb;
    if ((!a && na) || (!b && nb) || (!out && n)) return ADSB_E_ARG;
    adsb_ctx::Merge &m = c->merge;
    adsbk::MergeArgs g{};
    adsb_frame *out_use = nullptr;
    uint32_t *src_use = nullptr;
    if ((rc = stage_list(c, a, na, m.a, &g.a)) != ADSB_OK) return rc;
    if ((rc = stage_list(c, b, nb, m.b, &g.b)) != ADSB_OK) return rc;
    if ((rc = stage_result(c, out, n, m.out, &out_use)) != ADSB_OK) return rc;
    if ((rc = stage_result(c, src, n, m.src, &src_use)) != ADSB_OK) return rc;
    if ((rc = grow(c, m.prefix, prefix.size())) != ADSB_OK) return rc;
    HIPCHK(hipMemcpyAsync(m.prefix.p, prefix.data(), 8 * prefix.size(), hipMemcpyHostToDevice, c->aux));
    g.prefix_a = m.prefix.p, g.prefix_b = m.prefix.p + nc + 1;
    g.n_channels = n_channels, g.na = (uint32_t)na, g.nb = (uint32_t)nb;
    g.out = out_use, g.src = src_use;
    HIPCHK(adsbk::launch_merge_lists(c->aux, g));
    if (n && out_use != out) HIPCHK(hipMemcpyAsync(out, out_use, sizeof(adsb_frame) * n, hipMemcpyDeviceToHost, c->aux));
    if (n && src && src_use != src) HIPCHK(hipMemcpyAsync(src, src_use, 4 * n, hipMemcpyDeviceToHost, c->aux));
    if (counts_out) {
        for (size_t i = 0; i < nc; ++i) ca[i] += cb[i];
        if (in_device_memory(c, counts_out)) HIPCHK(hipMemcpyAsync(counts_out, ca.data(), 8 * nc, hipMemcpyHostToDevice, c->aux));
        else std::copy(ca.begin(), ca.end(), counts_out);
    }
    HIPCHK(hipStreamSynchronize(c->aux));
    return ADSB_OK;
}
