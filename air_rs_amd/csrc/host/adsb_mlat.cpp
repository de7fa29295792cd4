// adsb_mlat.cpp -- CPU mirror of the device's multilaterate (adsb_mlat.hip): adsb_host_multilaterate of
// include/adsb_host.h.  The solver is ../adsb_mlat.h, the text the device compiles; here the walk over the messages, the
// used mark, and the 16 partial sums a message's lanes hold on the device, folded in the same butterfly.  No device.
#include "../../../include/adsb_host.h"
#include "../adsb_mlat.h"

#include <vector>

namespace {

using namespace adsbk;

// One message's used receptions as the range rows see them, in reception order; k: the index inside the message.
struct MlatRows {
    struct Row {
        uint32_t k;
        double sx, sy, sz, rho;
    };
    std::vector<Row> rows;

    // the folded sums of the range rows at x: partial l takes the rows with k = l (mod 16) in ascending k
    void operator()(const double *x, MlatSums &s) const
    {
        MlatSums part[kMlatLanes];
        for (uint32_t l = 0; l < kMlatLanes; ++l) mlat_sums_zero(part[l]);
        for (const Row &r : rows) mlat_range_row(part[r.k % kMlatLanes], x, r.sx, r.sy, r.sz, r.rho);
        for (int i = 0; i < 15; ++i) {
            double v[kMlatLanes];
            for (uint32_t l = 0; l < kMlatLanes; ++l) v[l] = part[l].v[i];
            s.v[i] = mlat_fold16(v);
        }
    }
};

} // namespace

extern "C" int adsb_host_multilaterate(const adsb_mlat_cfg *cfg, const adsb_mlat_receiver *receivers, uint32_t n_receivers,
                                       const adsb_message *msgs, size_t n_msgs, const adsb_reception *recs, size_t n_recs,
                                       const adsb_wire_rx *rx, size_t n_rx, adsb_mlat_fix *fixes, adsb_mlat_header *header)
{
#pragma clang fp contract(off)
    if (!cfg || !receivers || n_receivers < 1 || n_receivers > kMlatMaxReceivers || !mlat_cfg_ok(*cfg)) return ADSB_E_ARG;
    if (cfg->time_source == ADSB_MLAT_TIME_TICKS && !rx) return ADSB_E_ARG;
    for (uint32_t r = 0; r < n_receivers; ++r)
        if (!mlat_receiver_ok(receivers[r])) return ADSB_E_ARG;
    if ((!msgs && n_msgs) || (!recs && n_recs) || (!rx && n_rx) || (!fixes && n_msgs)) return ADSB_E_ARG;
    if ((uint64_t)n_msgs > 0xFFFFFFFFull || (uint64_t)n_recs > 0xFFFFFFFFull || (uint64_t)n_rx > 0xFFFFFFFFull)
        return ADSB_E_CAPACITY;

    const MlatParams p = mlat_params_of(*cfg);
    const bool ticks = p.time_source == ADSB_MLAT_TIME_TICKS;
    std::vector<MlatStation> st(n_receivers);
    for (uint32_t r = 0; r < n_receivers; ++r) st[r] = mlat_station_of(receivers[r]);
    MlatCount total{0, 0, 0, 0};
    MlatRows rows;
    std::vector<uint8_t> seen(n_receivers);
    for (size_t g = 0; g < n_msgs; ++g) {
        const adsb_message &msg = msgs[g];
        const uint32_t n = msg.n_receptions;
        adsb_mlat_fix fix;
        bool bad = (uint64_t)msg.first + n > (uint64_t)n_recs;
        if (!bad && n <= ADSB_MLAT_MAX_RECEPTIONS)
            for (uint32_t k = 0; k < n; ++k) {
                const adsb_reception &r = recs[msg.first + k];
                if (r.receiver >= n_receivers || (ticks && r.frame >= n_rx)) bad = true;
            }
        if (bad) {
            fix = mlat_fix_empty(ADSB_MLAT_BAD_INDEX, 0);
        } else if (n > ADSB_MLAT_MAX_RECEPTIONS) {
            fix = mlat_fix_empty(ADSB_MLAT_TOO_MANY, 0);
        } else {
            const adsb_reception *mr = recs + msg.first;
            const auto time_of = [&](const adsb_reception &r) { return ticks ? rx[r.frame].ticks : r.time; };
            std::fill(seen.begin(), seen.end(), 0);
            rows.rows.clear();
            double cpart[3][kMlatLanes] = {};
            uint64_t t0 = 0;
            double clock0 = 0.0;
            for (uint32_t k = 0; k < n; ++k) {
                const adsb_reception &r = mr[k];
                if (seen[r.receiver]) continue; // an earlier reception of the message has this receiver
                seen[r.receiver] = 1;
                const MlatStation &q = st[r.receiver];
                if (k == 0) {
                    t0 = time_of(r);
                    clock0 = q.clock;
                }
                rows.rows.push_back(MlatRows::Row{k, q.x, q.y, q.z, mlat_rho(p, time_of(r), t0, q.clock, clock0)});
                cpart[0][k % kMlatLanes] += q.x;
                cpart[1][k % kMlatLanes] += q.y;
                cpart[2][k % kMlatLanes] += q.z;
            }
            const uint32_t n_used = (uint32_t)rows.rows.size();
            double alt_m = 0.0;
            const bool has_alt = (p.flags & ADSB_MLAT_USE_ALTITUDE) && mlat_altitude_of(msg.bytes, alt_m);
            if (n_used < mlat_need(p, has_alt)) {
                fix = mlat_fix_empty(ADSB_MLAT_TOO_FEW, n_used);
            } else {
                const double nu = (double)n_used;
                const double cen[3] = {mlat_fold16(cpart[0]) / nu, mlat_fold16(cpart[1]) / nu, mlat_fold16(cpart[2]) / nu};
                const MlatStation &q0 = st[mr[0].receiver];
                const double s0[3] = {q0.x, q0.y, q0.z};
                fix = mlat_solve_message(p, n_used, has_alt, alt_m, s0, cen, rows);
            }
        }
        fixes[g] = fix;
        total = mlat_count_add(total, mlat_count_of(fix.flags));
    }
    if (header) {
        header->n_messages = total.n_messages;
        header->n_attempted = total.n_attempted;
        header->n_valid = total.n_valid;
        header->flags = total.flags;
    }
    return (total.flags & ADSB_MLAT_HDR_BAD_INDEX) ? ADSB_E_ARG : ADSB_OK;
}
