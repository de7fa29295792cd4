// adsb_mlat_api.cpp -- the C boundary of multilaterate (include/adsb_hip.h, "Multilaterate"): argument checks, the
// stations' ECEF positions (computed here, on the host, by the text the CPU mirror uses), the one device block the
// results are carved from, the copies of host lists, and the fetch.  The kernel is adsb_mlat.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "adsb_mlat.h"
#include "adsb_scratch.h"

// One block for the fixes of `msgs` messages (at least one).  Every array starts 256-byte aligned.
static int mlat_reserve(adsb_ctx *c, size_t msgs)
{
    adsb_ctx::Mlat &k = c->mlat;
    if (k.mem.p && k.msgs >= msgs) return ADSB_OK;
    const size_t f = std::max<size_t>(msgs, 1);
    const size_t temp_bytes = adsbk::mlat_temp_bytes(f);
    k.done = false; // (what adsb_fetch_mlat would copy from goes)
    k.msgs = 0;
    if (temp_bytes == 0) return ADSB_E_NOMEM;
    const int rc = carve_block(c, k.mem, [&k, f, temp_bytes](Carve &cv) {
        k.fixes = cv.take<adsb_mlat_fix>(f);
        k.temp = cv.take<char>(temp_bytes);
        k.temp_bytes = temp_bytes;
        k.hdr = cv.take<adsb_mlat_header>(1);
        k.stations = cv.take<adsbk::MlatStation>(adsbk::kMlatMaxReceivers);
    });
    if (rc != ADSB_OK) return rc;
    k.msgs = f;
    return ADSB_OK;
}

static int mlat_check(const adsb_ctx *c, const adsb_mlat_cfg *cfg, const adsb_mlat_receiver *receivers, uint32_t n_receivers,
                      const void *rx)
{
    if (!c || !cfg || !receivers || n_receivers < 1 || n_receivers > adsbk::kMlatMaxReceivers) return ADSB_E_ARG;
    if (!adsbk::mlat_cfg_ok(*cfg)) return ADSB_E_ARG;
    if (cfg->time_source == ADSB_MLAT_TIME_TICKS && !rx) return ADSB_E_ARG;
    for (uint32_t r = 0; r < n_receivers; ++r)
        if (!adsbk::mlat_receiver_ok(receivers[r])) return ADSB_E_ARG;
    return ADSB_OK;
}

// The lists are device memory by now.  counts_dev: see MlatArgs.
static int mlat_run(adsb_ctx *c, const adsb_mlat_cfg &cfg, const adsb_mlat_receiver *receivers, uint32_t n_receivers,
                    adsbk::MlatArgs a)
{
    adsb_ctx::Mlat &k = c->mlat;
    const int rc = mlat_reserve(c, a.n_msgs);
    if (rc != ADSB_OK) return rc;
    std::vector<adsbk::MlatStation> st(n_receivers);
    for (uint32_t r = 0; r < n_receivers; ++r) st[r] = adsbk::mlat_station_of(receivers[r]);
    HIPCHK(hipMemcpyAsync(k.stations, st.data(), sizeof(adsbk::MlatStation) * n_receivers, hipMemcpyHostToDevice, c->aux));
    HIPCHK(hipStreamSynchronize(c->aux)); // the host arrays are this frame's (and the caller's) again
    a.n_receivers = n_receivers;
    a.stations = k.stations;
    a.p = adsbk::mlat_params_of(cfg);
    a.temp = k.temp;
    a.temp_bytes = k.temp_bytes;
    a.fixes = k.fixes;
    a.hdr = k.hdr;
    HIPCHK(adsbk::launch_mlat(c->aux, a));
    k.done = true;
    return ADSB_OK;
}

extern "C" int adsb_multilaterate_of(adsb_ctx *c, const adsb_mlat_cfg *cfg, const adsb_mlat_receiver *receivers,
                                     uint32_t n_receivers, const adsb_message *msgs, size_t n_msgs,
                                     const adsb_reception *recs, size_t n_recs, const adsb_wire_rx *rx, size_t n_rx)
{
    int rc = mlat_check(c, cfg, receivers, n_receivers, rx);
    if (rc != ADSB_OK) return rc;
    if ((!msgs && n_msgs) || (!recs && n_recs) || (!rx && n_rx)) return ADSB_E_ARG;
    if ((uint64_t)n_msgs > 0xFFFFFFFFull || (uint64_t)n_recs > 0xFFFFFFFFull || (uint64_t)n_rx > 0xFFFFFFFFull)
        return ADSB_E_CAPACITY;
    HIPCHK(hipSetDevice(c->cfg.device));
    adsb_ctx::Mlat &k = c->mlat;
    adsbk::MlatArgs a{};
    if ((rc = stage_list(c, msgs, n_msgs, k.in_msgs, &a.msgs)) != ADSB_OK) return rc;
    if ((rc = stage_list(c, recs, n_recs, k.in_recs, &a.recs)) != ADSB_OK) return rc;
    if ((rc = stage_list(c, rx, n_rx, k.in_rx, &a.rx)) != ADSB_OK) return rc;
    a.n_msgs = (uint32_t)n_msgs;
    a.n_recs = (uint32_t)n_recs;
    a.n_rx = (uint32_t)n_rx;
    return mlat_run(c, *cfg, receivers, n_receivers, a); // waits for the copies above before it returns
}

extern "C" int adsb_multilaterate(adsb_ctx *c, const adsb_mlat_cfg *cfg, const adsb_mlat_receiver *receivers,
                                  uint32_t n_receivers, const adsb_wire_rx *rx)
{
    int rc = mlat_check(c, cfg, receivers, n_receivers, rx);
    if (rc != ADSB_OK) return rc;
    const adsb_ctx::Corr &corr = c->corr;
    if (!corr.done) return ADSB_E_STATE;
    HIPCHK(hipSetDevice(c->cfg.device));
    adsb_ctx::Mlat &k = c->mlat;
    adsbk::MlatArgs a{};
    // the correlate result where it lies; its lengths are the header's, on the device: the list's n bounds both
    a.msgs = corr.a.msgs;
    a.recs = corr.a.recs;
    a.counts_dev = corr.a.hdr;
    a.n_msgs = a.n_recs = corr.n;
    if (rx) {
        if ((rc = stage_list(c, rx, (size_t)corr.n, k.in_rx, &a.rx)) != ADSB_OK) return rc;
        a.n_rx = corr.n;
    }
    return mlat_run(c, *cfg, receivers, n_receivers, a);
}

extern "C" int adsb_fetch_mlat(adsb_ctx *c, adsb_mlat_fix *fixes, size_t max, size_t *n, adsb_mlat_header *header)
{
    if (!c || (!fixes && max)) return ADSB_E_ARG;
    const adsb_ctx::Mlat &k = c->mlat;
    if (!k.done) return ADSB_E_STATE;
    HIPCHK(hipSetDevice(c->cfg.device));
    adsb_mlat_header h{};
    HIPCHK(hipMemcpyAsync(&h, k.hdr, sizeof(h), hipMemcpyDeviceToHost, c->aux));
    HIPCHK(hipStreamSynchronize(c->aux));
    const size_t take = std::min<size_t>((size_t)h.n_messages, max);
    if (take) HIPCHK(hipMemcpyAsync(fixes, k.fixes, sizeof(adsb_mlat_fix) * take, hipMemcpyDeviceToHost, c->aux));
    HIPCHK(hipStreamSynchronize(c->aux));
    if (n) *n = take;
    if (header) *header = h;
    return (h.flags & ADSB_MLAT_HDR_BAD_INDEX) ? ADSB_E_ARG : ADSB_OK;
}

extern "C" int adsb_mlat_device(adsb_ctx *c, const adsb_mlat_fix **fixes_dev, const void **header_dev)
{
    if (!c) return ADSB_E_ARG;
    const adsb_ctx::Mlat &k = c->mlat;
    if (!k.done) return ADSB_E_STATE;
    if (fixes_dev) *fixes_dev = k.fixes;
    if (header_dev) *header_dev = k.hdr;
    return ADSB_OK;
}

extern "C" int adsb_debug_mlat_geometry(uint32_t *lanes_per_message, uint32_t *messages_per_block)
{
    if (lanes_per_message) *lanes_per_message = adsbk::kMlatLanes;
    if (messages_per_block) *messages_per_block = adsbk::kMlatPerBlock;
    return ADSB_OK;
}
