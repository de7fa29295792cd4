// adsb_es_api.cpp -- the C boundary of the extended squitter status stage (include/adsb_hip.h, "Extended squitter
// status"): argument checks, the one device block the kernels' arrays are carved from, the copy of a host list, and the
// fetch.  The kernels are adsb_es.hip.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "adsb_es.h"
#include "adsb_scratch.h"

// One block for `frames` frames.  Every array starts 256-byte aligned.
static int es_reserve(adsb_ctx *c, size_t frames)
{
    adsb_ctx::Es &k = c->es;
    if (k.mem.p && k.frames >= frames) return ADSB_OK;
    const size_t f = std::max<size_t>(frames, 1);
    k.done = false;
    k.frames = 0;
    const int rc = carve_block(c, k.mem, [&k, f](Carve &cv) {
        adsbk::EsArgs &a = k.a;
        a = adsbk::EsArgs{};
        a.tally = cv.take<uint32_t>(adsbk::kEsTallyWords * (size_t)adsbk::es_blocks(f));
        a.recs = cv.take<adsb_es_rec>(f);
        a.hdr = cv.take<adsb_es_header>(1);
    });
    if (rc != ADSB_OK) return rc;
    k.frames = f;
    return ADSB_OK;
}

extern "C" int adsb_es_of(adsb_ctx *c, const adsb_frame *frames, size_t n)
{
    if (!c) return ADSB_E_ARG;
    HIPCHK(hipSetDevice(c->cfg.device));
    int rc = adsbk::es_args_check(frames, n);
    if (rc != ADSB_OK) return rc;
    adsb_ctx::Es &k = c->es;
    const adsb_frame *f_use = nullptr;
    if ((rc = stage_list(c, frames, n, k.in_frames, &f_use)) != ADSB_OK) return rc;
    if ((rc = es_reserve(c, n)) != ADSB_OK) return rc;
    adsbk::EsArgs a = k.a;
    a.frames = f_use;
    a.n = (uint32_t)n;
    HIPCHK(hipStreamSynchronize(c->aux)); // the host list is the caller's again
    HIPCHK(adsbk::launch_es(c->aux, a));
    k.done = true;
    return ADSB_OK;
}

extern "C" int adsb_fetch_es(adsb_ctx *c, adsb_es_rec *recs, size_t max_recs, adsb_es_header *header)
{
    if (!c || (!recs && max_recs)) return ADSB_E_ARG;
    const adsb_ctx::Es &k = c->es;
    if (!k.done) return ADSB_E_STATE;
    HIPCHK(hipSetDevice(c->cfg.device));
    adsb_es_header h{};
    HIPCHK(hipMemcpyAsync(&h, k.a.hdr, sizeof(h), hipMemcpyDeviceToHost, c->aux));
    HIPCHK(hipStreamSynchronize(c->aux));
    const size_t nr = std::min<size_t>((size_t)h.n, max_recs);
    if (nr) HIPCHK(hipMemcpyAsync(recs, k.a.recs, sizeof(adsb_es_rec) * nr, hipMemcpyDeviceToHost, c->aux));
    HIPCHK(hipStreamSynchronize(c->aux));
    if (header) *header = h;
    return ADSB_OK;
}

extern "C" int adsb_es_device(adsb_ctx *c, const adsb_es_rec **recs_dev, const void **header_dev)
{
    if (!c) return ADSB_E_ARG;
    const adsb_ctx::Es &k = c->es;
    if (!k.done) return ADSB_E_STATE;
    if (recs_dev) *recs_dev = k.a.recs;
    if (header_dev) *header_dev = k.a.hdr;
    return ADSB_OK;
}

extern "C" int adsb_debug_es_geometry(uint32_t *threads_per_block)
{
    if (threads_per_block) *threads_per_block = adsbk::kEsBlock;
    return ADSB_OK;
}
