// adsb_modes_api.cpp -- the C boundary of the Mode S stage (include/adsb_hip.h, "Mode S replies"): argument checks, the
// one device block the kernels' arrays are carved from, the copies of host lists, and the fetch.  The kernels are
// adsb_modes.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "adsb_modes.h"
#include "adsb_scratch.h"

// One block for `frames` frames and `known` entries of known_in.  Every array starts 256-byte aligned.
static int modes_reserve(adsb_ctx *c, size_t frames, size_t known)
{
    adsb_ctx::Modes &k = c->modes;
    if (k.mem.p && k.frames >= frames && k.known >= known) return ADSB_OK;
    frames = std::max(frames, k.frames);
    known = std::max(known, k.known);
    const size_t f = std::max<size_t>(frames, 1), m = f + known;
    const size_t temp_bytes = adsbk::modes_temp_bytes(m);
    k.done = false;
    k.frames = k.known = 0;
    if (temp_bytes == 0) return ADSB_E_NOMEM;
    const int rc = carve_block(c, k.mem, [&k, f, m, temp_bytes](Carve &cv) {
        adsbk::ModesArgs &a = k.a;
        a = adsbk::ModesArgs{};
        a.key = cv.take<uint32_t>(m);
        a.val = cv.take<uint32_t>(m);
        a.key_s = cv.take<uint32_t>(m);
        a.val_s = cv.take<uint32_t>(m);
        a.hidx = cv.take<uint32_t>(m);
        a.first = cv.take<uint32_t>(m);
        a.sidx = cv.take<uint32_t>(f);
        a.tally = cv.take<uint32_t>(5 * (size_t)adsbk::modes_blocks(f));
        a.temp = cv.take<char>(temp_bytes);
        a.temp_bytes = temp_bytes;
        a.recs = cv.take<adsb_modes_rec>(f);
        a.known_out = cv.take<uint32_t>(m);
        a.squitters = cv.take<adsb_frame>(f);
        a.sq_counts = cv.take<uint64_t>(adsbk::kModesMaxReceivers);
        a.hdr = cv.take<adsb_modes_header>(1);
        k.prefix = cv.take<uint64_t>(adsbk::kModesMaxReceivers + 1);
    });
    if (rc != ADSB_OK) return rc;
    k.frames = frames;
    k.known = known;
    return ADSB_OK;
}

// *use = a list the kernels may read while they write the block and while the block is replaced: a host list, or a
// result of the last call handed back in (known_out as the next known_in, squitters as the next frames), goes to b first
template <class T>
static int modes_stage(adsb_ctx *c, const T *src, size_t n, DevBuf<T> &b, const T **use)
{
    const adsb_ctx::Modes &k = c->modes;
    const char *p = reinterpret_cast<const char *>(src);
    if (src && n && k.mem.p && p >= k.mem.p && p < k.mem.p + k.mem.n) {
        const int rc = grow(c, b, n);
        if (rc != ADSB_OK) return rc;
        HIPCHK(hipMemcpyAsync(b.p, src, sizeof(T) * n, hipMemcpyDeviceToDevice, c->aux));
        *use = b.p;
        return ADSB_OK;
    }
    return stage_list(c, src, n, b, use);
}

extern "C" int adsb_modes_of(adsb_ctx *c, const adsb_frame *frames, size_t n, const uint64_t *counts, uint32_t n_receivers,
                             const uint32_t *known_in, size_t n_known_in)
{
    if (!c) return ADSB_E_ARG;
    HIPCHK(hipSetDevice(c->cfg.device));
    const bool known_host = n_known_in && known_in && !in_device_memory(c, known_in);
    int rc = adsbk::modes_args_check(frames, n, counts, n_receivers, known_in, n_known_in, known_host);
    if (rc != ADSB_OK) return rc;
    adsb_ctx::Modes &k = c->modes;
    const adsb_frame *f_use = nullptr;
    const uint32_t *k_use = nullptr;
    // (before the block may be replaced: a list inside it is copied out first, on the stream the replace waits for)
    if ((rc = modes_stage(c, frames, n, k.in_frames, &f_use)) != ADSB_OK) return rc;
    if ((rc = modes_stage(c, known_in, n_known_in, k.in_known, &k_use)) != ADSB_OK) return rc;
    if ((rc = modes_reserve(c, n, n_known_in)) != ADSB_OK) return rc;
    adsbk::ModesArgs a = k.a;
    a.frames = f_use;
    a.known_in = k_use;
    a.n = (uint32_t)n;
    a.n_known_in = (uint32_t)n_known_in;
    a.n_receivers = counts ? n_receivers : 0u;
    a.prefix = nullptr;
    if (counts) {
        std::vector<uint64_t> prefix((size_t)n_receivers + 1, 0);
        for (uint32_t r = 0; r < n_receivers; ++r) prefix[r + 1] = prefix[r] + counts[r];
        HIPCHK(hipMemcpyAsync(k.prefix, prefix.data(), sizeof(uint64_t) * prefix.size(), hipMemcpyHostToDevice, c->aux));
        HIPCHK(hipStreamSynchronize(c->aux)); // prefix is this frame's
        a.prefix = k.prefix;
    }
    HIPCHK(hipStreamSynchronize(c->aux)); // the host arrays are the caller's again
    HIPCHK(adsbk::launch_modes(c->aux, a));
    k.n_receivers = a.n_receivers;
    k.done = true;
    return ADSB_OK;
}

extern "C" int adsb_fetch_modes(adsb_ctx *c, adsb_modes_rec *recs, size_t max_recs, uint32_t *known_out, size_t max_known,
                                adsb_frame *squitters, size_t max_squitters, uint64_t *squitter_counts, uint32_t n_receivers,
                                adsb_modes_header *header)
{
    if (!c || (!recs && max_recs) || (!known_out && max_known) || (!squitters && max_squitters)) return ADSB_E_ARG;
    const adsb_ctx::Modes &k = c->modes;
    if (!k.done) return ADSB_E_STATE;
    if (n_receivers > k.n_receivers) return ADSB_E_ARG;
    HIPCHK(hipSetDevice(c->cfg.device));
    adsb_modes_header h{};
    HIPCHK(hipMemcpyAsync(&h, k.a.hdr, sizeof(h), hipMemcpyDeviceToHost, c->aux));
    HIPCHK(hipStreamSynchronize(c->aux));
    const size_t nr = std::min<size_t>((size_t)h.n, max_recs), nk = std::min<size_t>((size_t)h.n_known_out, max_known),
                 ns = std::min<size_t>((size_t)h.n_squitters, max_squitters);
    if (nr) HIPCHK(hipMemcpyAsync(recs, k.a.recs, sizeof(adsb_modes_rec) * nr, hipMemcpyDeviceToHost, c->aux));
    if (nk) HIPCHK(hipMemcpyAsync(known_out, k.a.known_out, sizeof(uint32_t) * nk, hipMemcpyDeviceToHost, c->aux));
    if (ns) HIPCHK(hipMemcpyAsync(squitters, k.a.squitters, sizeof(adsb_frame) * ns, hipMemcpyDeviceToHost, c->aux));
    if (n_receivers && squitter_counts)
        HIPCHK(hipMemcpyAsync(squitter_counts, k.a.sq_counts, 8 * (size_t)n_receivers, hipMemcpyDeviceToHost, c->aux));
    HIPCHK(hipStreamSynchronize(c->aux));
    if (header) *header = h;
    return ADSB_OK;
}

extern "C" int adsb_modes_device(adsb_ctx *c, const adsb_modes_rec **recs_dev, const uint32_t **known_out_dev,
                                 const adsb_frame **squitters_dev, const uint64_t **squitter_counts_dev,
                                 const void **header_dev)
{
    if (!c) return ADSB_E_ARG;
    const adsb_ctx::Modes &k = c->modes;
    if (!k.done) return ADSB_E_STATE;
    if (recs_dev) *recs_dev = k.a.recs;
    if (known_out_dev) *known_out_dev = k.a.known_out;
    if (squitters_dev) *squitters_dev = k.a.squitters;
    if (squitter_counts_dev) *squitter_counts_dev = k.n_receivers ? k.a.sq_counts : nullptr;
    if (header_dev) *header_dev = k.a.hdr;
    return ADSB_OK;
}

extern "C" int adsb_debug_modes_geometry(uint32_t *threads_per_block)
{
    if (threads_per_block) *threads_per_block = adsbk::kModesBlock;
    return ADSB_OK;
}
