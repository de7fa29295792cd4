// adsb_correlate.cpp -- CPU mirror of the device's correlate (adsb_correlate.hip): adsb_host_correlate of
// include/adsb_host.h.  The key compare, the head rule and the aggregate's combine are ../adsb_correlate.h, the text the
// device compiles; here the two sorts and the walk over the groups.  No device.
#include "../../../include/adsb_host.h"
#include "../adsb_correlate.h"

#include <algorithm>
#include <vector>

extern "C" int adsb_host_correlate(const adsb_correlate_cfg *cfg, const adsb_frame *frames, const adsb_frame_level *levels,
                                   size_t n, const uint64_t *counts, uint32_t n_receivers, const uint64_t *sample_base,
                                   adsb_message *msgs, size_t max_msgs, size_t *n_msgs, adsb_frame *frames_out,
                                   adsb_reception *recs)
{
    using namespace adsbk;
    if (!cfg || !counts || n_receivers < 1 || n_receivers > kCorrMaxReceivers || (!frames && n) || (!recs && n) ||
        !n_msgs)
        return ADSB_E_ARG;
    if ((uint64_t)n > 0xFFFFFFFFull) return ADSB_E_CAPACITY;
    uint64_t sum = 0;
    for (uint32_t r = 0; r < n_receivers; ++r) {
        if (counts[r] > (uint64_t)n - sum) return ADSB_E_ARG;
        sum += counts[r];
    }
    if (sum != (uint64_t)n) return ADSB_E_ARG;

    std::vector<CorrRec> rec(n);
    std::vector<uint16_t> rx(n);
    size_t j = 0;
    for (uint32_t r = 0; r < n_receivers; ++r)
        for (uint64_t k = 0; k < counts[r]; ++k, ++j) {
            rec[j] = CorrRec{(sample_base ? sample_base[r] : 0ull) + frames[j].offset, corr_key_lo(frames[j].bytes),
                             corr_key_hi(frames[j].bytes)};
            rx[j] = (uint16_t)r;
        }
    std::vector<uint32_t> ord(n);
    for (size_t p = 0; p < n; ++p) ord[p] = (uint32_t)p;
    std::sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) { return corr_before(rec[a], a, rec[b], b); });

    // the groups in group order: where each starts in ord[], and its aggregate
    struct Group {
        size_t at;
        CorrAgg agg;
    };
    std::vector<Group> groups;
    for (size_t p = 0; p < n; ++p) {
        const uint32_t i = ord[p];
        const bool head = p == 0 || corr_is_head(rec[ord[p - 1]], rec[i], cfg->window);
        const CorrAgg one = corr_agg_of(rec[i].t, rx[i], frames[i], levels ? levels + i : nullptr, head);
        if (head) groups.push_back(Group{p, one});
        else groups.back().agg = corr_combine(groups.back().agg, one);
    }
    // message order: by time; group order, kept inside equal times, is ascending K there
    std::stable_sort(groups.begin(), groups.end(),
                     [](const Group &a, const Group &b) { return a.agg.first_t < b.agg.first_t; });
    size_t q = 0;
    for (size_t m = 0; m < groups.size(); ++m) {
        const Group &g = groups[m];
        const adsb_message msg = corr_message_of(g.agg, frames[ord[g.at]].bytes, (uint32_t)q);
        if (m < max_msgs) {
            if (msgs) msgs[m] = msg;
            if (frames_out) frames_out[m] = corr_frame_of(msg);
        }
        for (uint32_t k = 0; k < g.agg.n; ++k, ++q) {
            const uint32_t i = ord[g.at + k];
            recs[q] = adsb_reception{rec[i].t, i, rx[i], 0};
        }
    }
    *n_msgs = groups.size();
    return ADSB_OK;
}
