// adsb_clock_api.cpp -- the C boundary of clock sync (include/adsb_hip.h, "Clock sync"): argument checks, the stations'
// ECEF positions (computed here, on the host, by the text the CPU mirror uses), the one device block the scratch and the
// results are carved from, the copies of host lists, apply, and the fetches.  The kernels are adsb_clock.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "adsb_clock.h"
#include "adsb_scratch.h"

// One block for lists of `msgs` messages and `recs` receptions (at least one each).  Every array starts 256-byte
// aligned.
static int clock_reserve(adsb_ctx *c, size_t msgs, size_t recs)
{
    adsb_ctx::Clock &k = c->clock;
    if (k.mem.p && k.msgs >= msgs && k.recs >= recs) return ADSB_OK;
    const size_t m = std::max<size_t>(std::max(msgs, k.msgs), 1), r = std::max<size_t>(std::max(recs, k.recs), 1);
    const size_t temp_bytes = adsbk::clock_temp_bytes(r);
    k.done = k.applied = false; // (what the fetches would copy from goes)
    k.msgs = k.recs = 0;
    if (temp_bytes == 0) return ADSB_E_NOMEM;
    adsbk::ClockArgs &a = k.a;
    const int rc = carve_block(c, k.mem, [&a, m, r, temp_bytes](Carve &cv) {
        a.tau = cv.take<double>(r);
        a.yp = cv.take<double>(r);
        a.key = cv.take<uint32_t>(r);
        a.key_sorted = cv.take<uint32_t>(r);
        a.slot_sorted = cv.take<uint32_t>(r);
        a.corrected = cv.take<adsb_reception>(r);
        a.msg_flags = cv.take<uint8_t>(m);
        a.temp = cv.take<char>(temp_bytes);
        a.temp_bytes = temp_bytes;
        a.pairs = cv.take<adsbk::ClockPair>(65536);
        a.pairs_first = cv.take<adsbk::ClockPair>(65536);
        a.normal = cv.take<double>((size_t)adsbk::kClockMaxUnknowns * adsbk::kClockMaxUnknowns);
        a.sol = cv.take<adsbk::ClockSol>(adsbk::kMlatMaxReceivers);
        a.stations = cv.take<adsbk::ClockStation>(adsbk::kMlatMaxReceivers);
        a.clocks = cv.take<adsb_clock>(adsbk::kMlatMaxReceivers);
        a.hdr = cv.take<adsb_clock_header>(1);
    });
    if (rc != ADSB_OK) return rc;
    k.msgs = m;
    k.recs = r;
    return ADSB_OK;
}

static int clock_check(const adsb_ctx *c, const adsb_clock_cfg *cfg, const adsb_mlat_receiver *receivers,
                       uint32_t n_receivers, const void *rx)
{
    if (!c || !cfg || !receivers || n_receivers < 1 || n_receivers > adsbk::kMlatMaxReceivers) return ADSB_E_ARG;
    if (!adsbk::clock_cfg_ok(*cfg, n_receivers)) return ADSB_E_ARG;
    if (cfg->time_source == ADSB_MLAT_TIME_TICKS && !rx) return ADSB_E_ARG;
    for (uint32_t r = 0; r < n_receivers; ++r)
        if (!adsbk::mlat_receiver_ok(receivers[r])) return ADSB_E_ARG;
    return ADSB_OK;
}

// The lists (in `in`) are device memory by now.
static int clock_run(adsb_ctx *c, const adsb_clock_cfg &cfg, const adsb_mlat_receiver *receivers, uint32_t n_receivers,
                     const adsbk::ClockArgs &in)
{
    adsb_ctx::Clock &k = c->clock;
    const int rc = clock_reserve(c, in.n_msgs, in.n_recs);
    if (rc != ADSB_OK) return rc;
    k.done = k.applied = false;
    adsbk::ClockArgs &a = k.a;
    a.msgs = in.msgs;
    a.recs = in.recs;
    a.rx = in.rx;
    a.counts_dev = in.counts_dev;
    a.n_msgs = in.n_msgs;
    a.n_recs = in.n_recs;
    a.n_rx = in.n_rx;
    a.n_receivers = n_receivers;
    a.p = adsbk::clock_params_of(cfg);
    std::vector<adsbk::ClockStation> st(n_receivers);
    for (uint32_t r = 0; r < n_receivers; ++r)
        st[r] = adsbk::ClockStation{adsbk::mlat_station_of(receivers[r]), receivers[r].latitude, receivers[r].longitude};
    HIPCHK(hipMemcpyAsync(const_cast<adsbk::ClockStation *>(a.stations), st.data(),
                          sizeof(adsbk::ClockStation) * n_receivers, hipMemcpyHostToDevice, c->aux));
    HIPCHK(hipStreamSynchronize(c->aux)); // the host arrays are this frame's (and the caller's) again
    HIPCHK(adsbk::launch_clock_sync(c->aux, a));
    k.done = true;
    return ADSB_OK;
}

extern "C" int adsb_clock_sync_of(adsb_ctx *c, const adsb_clock_cfg *cfg, const adsb_mlat_receiver *receivers,
                                  uint32_t n_receivers, const adsb_message *msgs, size_t n_msgs,
                                  const adsb_reception *recs, size_t n_recs, const adsb_wire_rx *rx, size_t n_rx)
{
    int rc = clock_check(c, cfg, receivers, n_receivers, rx);
    if (rc != ADSB_OK) return rc;
    if ((!msgs && n_msgs) || (!recs && n_recs) || (!rx && n_rx)) return ADSB_E_ARG;
    if ((uint64_t)n_msgs > 0xFFFFFFFFull || (uint64_t)n_recs > 0xFFFFFFFFull || (uint64_t)n_rx > 0xFFFFFFFFull)
        return ADSB_E_CAPACITY;
    HIPCHK(hipSetDevice(c->cfg.device));
    adsb_ctx::Clock &k = c->clock;
    adsbk::ClockArgs a{};
    if ((rc = stage_list(c, msgs, n_msgs, k.in_msgs, &a.msgs)) != ADSB_OK) return rc;
    if ((rc = stage_list(c, recs, n_recs, k.in_recs, &a.recs)) != ADSB_OK) return rc;
    if ((rc = stage_list(c, rx, n_rx, k.in_rx, &a.rx)) != ADSB_OK) return rc;
    a.n_msgs = (uint32_t)n_msgs;
    a.n_recs = (uint32_t)n_recs;
    a.n_rx = (uint32_t)n_rx;
    return clock_run(c, *cfg, receivers, n_receivers, a); // waits for the copies above before it returns
}

extern "C" int adsb_clock_sync(adsb_ctx *c, const adsb_clock_cfg *cfg, const adsb_mlat_receiver *receivers,
                               uint32_t n_receivers, const adsb_wire_rx *rx)
{
    int rc = clock_check(c, cfg, receivers, n_receivers, rx);
    if (rc != ADSB_OK) return rc;
    const adsb_ctx::Corr &corr = c->corr;
    if (!corr.done) return ADSB_E_STATE;
    HIPCHK(hipSetDevice(c->cfg.device));
    adsb_ctx::Clock &k = c->clock;
    adsbk::ClockArgs a{};
    // the correlate result where it lies; its lengths are the header's, on the device: the list's n bounds both
    a.msgs = corr.a.msgs;
    a.recs = corr.a.recs;
    a.counts_dev = corr.a.hdr;
    a.n_msgs = a.n_recs = corr.n;
    if (rx) {
        if ((rc = stage_list(c, rx, (size_t)corr.n, k.in_rx, &a.rx)) != ADSB_OK) return rc;
        a.n_rx = corr.n;
    }
    return clock_run(c, *cfg, receivers, n_receivers, a);
}

extern "C" int adsb_fetch_clocks(adsb_ctx *c, adsb_clock *clocks, size_t max, size_t *n, adsb_clock_header *header)
{
    if (!c || (!clocks && max)) return ADSB_E_ARG;
    const adsb_ctx::Clock &k = c->clock;
    if (!k.done) return ADSB_E_STATE;
    HIPCHK(hipSetDevice(c->cfg.device));
    adsb_clock_header h{};
    const size_t take = std::min<size_t>((size_t)k.a.n_receivers, max);
    HIPCHK(hipMemcpyAsync(&h, k.a.hdr, sizeof(h), hipMemcpyDeviceToHost, c->aux));
    if (take) HIPCHK(hipMemcpyAsync(clocks, k.a.clocks, sizeof(adsb_clock) * take, hipMemcpyDeviceToHost, c->aux));
    HIPCHK(hipStreamSynchronize(c->aux));
    if (n) *n = take;
    if (header) *header = h;
    return (h.flags & ADSB_CLOCK_HDR_BAD_INDEX) ? ADSB_E_ARG : ADSB_OK;
}

extern "C" int adsb_clocks_device(adsb_ctx *c, const adsb_clock **clocks_dev, const void **header_dev)
{
    if (!c) return ADSB_E_ARG;
    const adsb_ctx::Clock &k = c->clock;
    if (!k.done) return ADSB_E_STATE;
    if (clocks_dev) *clocks_dev = k.a.clocks;
    if (header_dev) *header_dev = k.a.hdr;
    return ADSB_OK;
}

extern "C" int adsb_clock_apply(adsb_ctx *c)
{
    if (!c) return ADSB_E_ARG;
    adsb_ctx::Clock &k = c->clock;
    if (!k.done) return ADSB_E_STATE;
    HIPCHK(hipSetDevice(c->cfg.device));
    HIPCHK(adsbk::launch_clock_apply(c->aux, k.a));
    k.applied = true;
    return ADSB_OK;
}

extern "C" int adsb_fetch_clock_receptions(adsb_ctx *c, adsb_reception *corrected, size_t max, size_t *n, size_t *n_total)
{
    if (!c || (!corrected && max)) return ADSB_E_ARG;
    const adsb_ctx::Clock &k = c->clock;
    if (!k.applied) return ADSB_E_STATE;
    HIPCHK(hipSetDevice(c->cfg.device));
    size_t total = k.a.n_recs;
    if (k.a.counts_dev) {
        uint64_t counts[2] = {0, 0};
        HIPCHK(hipMemcpyAsync(counts, k.a.counts_dev, sizeof(counts), hipMemcpyDeviceToHost, c->aux));
        HIPCHK(hipStreamSynchronize(c->aux));
        total = std::min<size_t>(total, (size_t)counts[1]);
    }
    const size_t take = std::min(total, max);
    if (take) HIPCHK(hipMemcpyAsync(corrected, k.a.corrected, sizeof(adsb_reception) * take, hipMemcpyDeviceToHost, c->aux));
    HIPCHK(hipStreamSynchronize(c->aux));
    if (n) *n = take;
    if (n_total) *n_total = total;
    return ADSB_OK;
}

extern "C" int adsb_clock_receptions_device(adsb_ctx *c, const adsb_reception **corrected_dev, size_t *n)
{
    if (!c) return ADSB_E_ARG;
    const adsb_ctx::Clock &k = c->clock;
    if (!k.applied) return ADSB_E_STATE;
    if (corrected_dev) *corrected_dev = k.a.corrected;
    if (n) *n = k.a.n_recs;
    return ADSB_OK;
}

extern "C" int adsb_debug_clock_geometry(uint32_t *messages_per_block, uint32_t *pair_partials)
{
    if (messages_per_block) *messages_per_block = adsbk::kClockPerBlock;
    if (pair_partials) *pair_partials = adsbk::kClockPartials;
    return ADSB_OK;
}
