// adsb_clock.cpp -- CPU mirror of the device's clock sync (adsb_clock.hip): adsb_host_clock_sync and
// adsb_host_clock_apply of include/adsb_host.h.  The text is ../adsb_clock.h, which the device compiles too; here the
// walk over the messages, the stable order of the rows, the 64 partial sums a pair's wavefront holds on the device, folded
// in the same butterfly, the hop labels, and the factorisation's columns one entry at a time.  No device.
#include "../../../include/adsb_host.h"
#include "../adsb_clock.h"

#include <algorithm>
#include <vector>

namespace {

using namespace adsbk;

struct ClockLists {
    ClockParams p;
    const adsb_message *msgs;
    size_t n_msgs;
    const adsb_reception *recs;
    size_t n_recs;
    const adsb_wire_rx *rx;
    size_t n_rx;
    uint32_t R;
    bool ticks() const { return p.time_source == ADSB_MLAT_TIME_TICKS; }
    uint64_t time_of(const adsb_reception &r) const { return ticks() ? rx[r.frame].ticks : r.time; }
};

int clock_lists_ok(const adsb_clock_cfg *cfg, uint32_t n_receivers, const adsb_message *msgs, size_t n_msgs,
                   const adsb_reception *recs, size_t n_recs, const adsb_wire_rx *rx, size_t n_rx)
{
    if (!cfg || n_receivers < 1 || n_receivers > kMlatMaxReceivers || !clock_cfg_ok(*cfg, n_receivers)) return ADSB_E_ARG;
    if (cfg->time_source == ADSB_MLAT_TIME_TICKS && !rx) return ADSB_E_ARG;
    if ((!msgs && n_msgs) || (!recs && n_recs) || (!rx && n_rx)) return ADSB_E_ARG;
    if ((uint64_t)n_msgs > 0xFFFFFFFFull || (uint64_t)n_recs > 0xFFFFFFFFull || (uint64_t)n_rx > 0xFFFFFFFFull)
        return ADSB_E_CAPACITY;
    return ADSB_OK;
}

// The pairs' sums over the rows whose key is not empty, in (pair, slot) order.
void clock_sums(const std::vector<uint32_t> &key, const std::vector<double> &tau, const std::vector<double> &yp,
                std::vector<ClockPair> &pairs)
{
#pragma clang fp contract(off)
    std::fill(pairs.begin(), pairs.end(), ClockPair{0.0, 0.0, 0.0, 0.0, 0.0, 0});
    std::vector<uint32_t> order;
    for (uint32_t s = 0; s < key.size(); ++s)
        if (key[s] <= 0xFFFFu) order.push_back(s);
    std::stable_sort(order.begin(), order.end(), [&key](uint32_t x, uint32_t y) { return key[x] < key[y]; });
    for (size_t begin = 0; begin < order.size();) {
        size_t end = begin;
        while (end < order.size() && key[order[end]] == key[order[begin]]) ++end;
        ClockPart part[kClockPartials];
        for (uint32_t l = 0; l < kClockPartials; ++l) clock_part_zero(part[l]);
        for (size_t q = 0; q < end - begin; ++q)
            clock_part_add(part[q % kClockPartials], tau[order[begin + q]], yp[order[begin + q]]);
        double folded[5];
        for (int i = 0; i < 5; ++i) {
            double v[kClockPartials];
            for (uint32_t l = 0; l < kClockPartials; ++l) v[l] = part[l].v[i];
            folded[i] = clock_fold64(v);
        }
        pairs[key[order[begin]]] = ClockPair{folded[0], folded[1], folded[2], folded[3], folded[4], end - begin};
        begin = end;
    }
}

// One solve of `stride` unknowns per receiver; the result in v.  false: a pivot failed.
bool clock_solve_system(const ClockParams &p, const std::vector<ClockPair> &pairs, uint32_t R,
                        const std::vector<uint32_t> &rcv_of, uint32_t stride, std::vector<double> &m,
                        std::vector<double> &v)
{
#pragma clang fp contract(off)
    const uint32_t n = (uint32_t)rcv_of.size() * stride;
    m.assign((size_t)n * n, 0.0);
    v.assign(n, 0.0);
    std::vector<double> d(n);
    for (uint32_t i = 0; i < n; ++i) {
        for (uint32_t j = 0; j <= i; ++j)
            m[(size_t)i * n + j] =
                clock_normal_entry(p, pairs.data(), R, rcv_of[i / stride], i % stride, rcv_of[j / stride], j % stride);
        v[i] = clock_rhs_entry(p, pairs.data(), R, rcv_of[i / stride], i % stride);
    }
    for (uint32_t j = 0; j < n; ++j) {
        d[j] = clock_ldl_entry(m.data(), d.data(), n, j, j);
        if (!clock_pivot_ok(d[j], m[(size_t)j * n + j])) return false;
        for (uint32_t i = j + 1; i < n; ++i) m[(size_t)i * n + j] = clock_ldl_entry(m.data(), d.data(), n, i, j) / d[j];
    }
    for (uint32_t k = 0; k < n; ++k)
        for (uint32_t i = k + 1; i < n; ++i) v[i] = v[i] - m[(size_t)i * n + k] * v[k];
    for (uint32_t i = 0; i < n; ++i) v[i] = v[i] / d[i];
    for (uint32_t k = n; k-- > 0;)
        for (uint32_t i = 0; i < k; ++i) v[i] = v[i] - m[(size_t)k * n + i] * v[k];
    return true;
}

// Reached set, solve and records of one pass -> the header's n_reached and solve flags.
uint64_t clock_solve(const ClockParams &p, const std::vector<ClockPair> &pairs, const std::vector<ClockPair> &first,
                     const std::vector<ClockStation> &st, std::vector<ClockSol> &sol, adsb_clock *clocks,
                     uint64_t &n_reached)
{
    const uint32_t R = (uint32_t)st.size();
    std::vector<uint8_t> reached(R, 0);
    reached[p.reference] = 1;
    for (uint32_t round = 1; round < R; ++round) { // one hop per round
        std::vector<uint8_t> next = reached;
        bool changed = false;
        for (uint32_t r = 0; r < R; ++r) {
            if (reached[r]) continue;
            for (uint32_t w = 0; w < R; ++w)
                if (reached[w] && clock_edge(p, pairs.data(), r, w)) next[r] = 1;
            changed = changed || next[r];
        }
        reached = next;
        if (!changed) break;
    }
    std::vector<uint32_t> rcv_of, unk(R, 0xFFFFFFFFu);
    for (uint32_t r = 0; r < R; ++r)
        if (r != p.reference && reached[r]) {
            unk[r] = (uint32_t)rcv_of.size();
            rcv_of.push_back(r);
        }
    n_reached = rcv_of.size() + 1;
    uint64_t flags = 0;
    std::vector<double> m, v;
    uint32_t stride = (p.flags & ADSB_CLOCK_DRIFT) ? 2u : 1u;
    bool solved = clock_solve_system(p, pairs, R, rcv_of, stride, m, v);
    if (!solved && stride == 2u) {
        flags |= ADSB_CLOCK_HDR_DRIFT_DROPPED;
        stride = 1u;
        solved = clock_solve_system(p, pairs, R, rcv_of, stride, m, v);
    }
    if (!solved) flags |= ADSB_CLOCK_HDR_SINGULAR;
    for (uint32_t r = 0; r < R; ++r) {
        sol[r] = ClockSol{0.0, 0.0};
        if (solved && unk[r] != 0xFFFFFFFFu) {
            sol[r].a = v[unk[r] * stride];
            if (stride == 2u) sol[r].b = v[unk[r] * stride + 1u];
        }
    }
    for (uint32_t r = 0; r < R; ++r)
        clocks[r] = clock_record(p, pairs.data(), first.data(), R, r, sol.data(), st[r].s.clock, reached[r] != 0,
                                 solved && stride == 2u);
    return flags;
}

} // namespace

extern "C" int adsb_host_clock_sync(const adsb_clock_cfg *cfg, const adsb_mlat_receiver *receivers, uint32_t n_receivers,
                                    const adsb_message *msgs, size_t n_msgs, const adsb_reception *recs, size_t n_recs,
                                    const adsb_wire_rx *rx, size_t n_rx, adsb_clock *clocks, adsb_clock_header *header,
                                    uint8_t *row_state)
{
#pragma clang fp contract(off)
    const int rc = clock_lists_ok(cfg, n_receivers, msgs, n_msgs, recs, n_recs, rx, n_rx);
    if (rc != ADSB_OK) return rc;
    if (!receivers || !clocks) return ADSB_E_ARG;
    for (uint32_t r = 0; r < n_receivers; ++r)
        if (!mlat_receiver_ok(receivers[r])) return ADSB_E_ARG;

    const ClockLists L{clock_params_of(*cfg), msgs, n_msgs, recs, n_recs, rx, n_rx, n_receivers};
    std::vector<ClockStation> st(n_receivers);
    for (uint32_t r = 0; r < n_receivers; ++r)
        st[r] = ClockStation{mlat_station_of(receivers[r]), receivers[r].latitude, receivers[r].longitude};
    std::vector<uint32_t> key(n_recs, kClockEmpty);
    std::vector<double> tau(n_recs, 0.0), yp(n_recs, 0.0);
    std::vector<uint8_t> seen(n_receivers), used;
    adsb_clock_header h{};
    h.n_messages = n_msgs;
    for (size_t g = 0; g < n_msgs; ++g) {
        const adsb_message &msg = msgs[g];
        const uint32_t n = msg.n_receptions;
        if ((uint64_t)msg.first + n > (uint64_t)n_recs) {
            h.flags |= ADSB_CLOCK_HDR_BAD_INDEX;
            continue;
        }
        if (n > ADSB_MLAT_MAX_RECEPTIONS) continue;
        const adsb_reception *mr = recs + msg.first;
        bool bad = false;
        for (uint32_t k = 0; k < n; ++k)
            if (mr[k].receiver >= n_receivers || (L.ticks() && mr[k].frame >= n_rx)) bad = true;
        if (bad) {
            h.flags |= ADSB_CLOCK_HDR_BAD_INDEX;
            continue;
        }
        std::fill(seen.begin(), seen.end(), 0);
        used.assign(n, 0);
        uint32_t n_used = 0;
        for (uint32_t k = 0; k < n; ++k) {
            if (seen[mr[k].receiver]) continue; // an earlier reception of the message has this receiver
            seen[mr[k].receiver] = 1;
            used[k] = 1;
            ++n_used;
        }
        if (n_used < 2) continue;
        const ClockStation &q0 = st[mr[0].receiver];
        double p[3];
        if (!clock_position(L.p, q0, msg.bytes, p)) continue;
        ++h.n_eligible;
        const uint64_t t0 = L.time_of(mr[0]);
        const double tau_m = clock_tau(msg.time, msgs[0].time, L.p.seconds_per_time);
        for (uint32_t k = 1; k < n; ++k) {
            if (!used[k]) continue;
            const MlatStation &q = st[mr[k].receiver].s;
            const double y = clock_row_y(L.p, mlat_dticks(L.p.time_source, L.time_of(mr[k]), t0), q0.s, q, p);
            const size_t slot = (size_t)msg.first + k;
            key[slot] = clock_key(mr[0].receiver, mr[k].receiver, y, yp[slot]);
            tau[slot] = tau_m;
        }
    }

    std::vector<ClockPair> first(65536), pairs;
    std::vector<ClockSol> sol(n_receivers);
    clock_sums(key, tau, yp, first);
    uint64_t n_reached = 0;
    uint64_t flags = clock_solve(L.p, first, first, st, sol, clocks, n_reached);
    if (row_state)
        for (size_t s = 0; s < n_recs; ++s) row_state[s] = key[s] <= 0xFFFFu ? 1 : 0;
    for (size_t s = 0; s < n_recs; ++s) h.n_rows += key[s] <= 0xFFFFu ? 1 : 0;
    if (L.p.max_residual_s > 0.0 && n_recs) {
        for (size_t s = 0; s < n_recs; ++s) {
            if (key[s] > 0xFFFFu) continue;
            const double r = clock_residual(yp[s], tau[s], sol[key[s] >> 8], sol[key[s] & 0xFFu]);
            if (fabs(r) > L.p.max_residual_s) {
                key[s] = kClockEmpty;
                ++h.n_dropped;
                if (row_state) row_state[s] = 2;
            }
        }
        pairs.resize(65536);
        clock_sums(key, tau, yp, pairs);
        flags = clock_solve(L.p, pairs, first, st, sol, clocks, n_reached);
    }
    h.n_reached = n_reached;
    h.flags |= flags;
    if (header) *header = h;
    return (h.flags & ADSB_CLOCK_HDR_BAD_INDEX) ? ADSB_E_ARG : ADSB_OK;
}

extern "C" int adsb_host_clock_apply(const adsb_clock_cfg *cfg, const adsb_clock *clocks, uint32_t n_receivers,
                                     const adsb_message *msgs, size_t n_msgs, const adsb_reception *recs, size_t n_recs,
                                     const adsb_wire_rx *rx, size_t n_rx, adsb_reception *corrected)
{
#pragma clang fp contract(off)
    const int rc = clock_lists_ok(cfg, n_receivers, msgs, n_msgs, recs, n_recs, rx, n_rx);
    if (rc != ADSB_OK) return rc;
    if (!clocks || (!corrected && n_recs)) return ADSB_E_ARG;
    const ClockLists L{clock_params_of(*cfg), msgs, n_msgs, recs, n_recs, rx, n_rx, n_receivers};
    for (size_t s = 0; s < n_recs; ++s) corrected[s] = recs[s];
    if (!n_msgs) return ADSB_OK;
    const adsb_message &m0 = msgs[0];
    uint64_t ref = 0;
    if (m0.n_receptions && (uint64_t)m0.first + m0.n_receptions <= (uint64_t)n_recs) {
        const adsb_reception &r = recs[m0.first];
        if (!L.ticks() || r.frame < n_rx) ref = L.time_of(r);
    }
    for (size_t g = 0; g < n_msgs; ++g) {
        const adsb_message &msg = msgs[g];
        if ((uint64_t)msg.first + msg.n_receptions > (uint64_t)n_recs) continue;
        const double tau = clock_tau(msg.time, m0.time, L.p.seconds_per_time);
        for (uint32_t k = 0; k < msg.n_receptions; ++k) {
            const adsb_reception &r = recs[msg.first + k];
            if (r.receiver >= n_receivers || (L.ticks() && r.frame >= n_rx)) continue; // keeps its raw time
            corrected[msg.first + k].time = clock_apply_time(mlat_dticks(L.p.time_source, L.time_of(r), ref),
                                                             clocks[r.receiver].offset_s, clocks[r.receiver].drift, tau,
                                                             L.p.seconds_per_tick);
        }
    }
    return ADSB_OK;
}
