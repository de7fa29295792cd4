// clock_edges.cpp -- stand-alone sanitizer run of the CPU mirror of clock sync (adsb_host_clock_sync and
// adsb_host_clock_apply, air_rs_amd/csrc/host/adsb_clock.cpp over air_rs_amd/csrc/adsb_clock.h, the text the device
// compiles too).  Exact-size heap buffers, so that one record past clocks[R], corrected[N] or row_state[N], or one
// reception read past recs[n_recs], is a heap-buffer-overflow; messages of 0, 1 and 2 receptions; a single message (the
// drift cannot be told and is dropped); stations all equal (no division by zero, no NaN in a decision); ticks that wrap at
// 2^48; 256 receivers (510 unknowns); indices the lists do not have (receiver, reception range, frame), which must be
// reported and never read; the empty list.  Every result is checked against what the definition says.  Host sources
// only, no device (-ffp-contract=off because g++ does not know the sources' `#pragma clang fp contract(off)`):
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/host/clock_edges.cpp air_rs_amd/csrc/host/adsb_clock.cpp -o /tmp/clock_edges && /tmp/clock_edges
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/adsb_host.h"

static int fails = 0;
#define CHECK(x)                                                     \
    do {                                                             \
        if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); ++fails; } \
    } while (0)

static const double kPi = 3.14159265358979323846, kA = 6378137.0, kE2 = 6.69437999014e-3, kRad = kPi / 180.0;

struct P3 {
    double x, y, z;
};

static P3 ecef(double lat, double lon, double h)
{
    const double sp = std::sin(lat * kRad), cp = std::cos(lat * kRad);
    const double n = kA / std::sqrt(1.0 - kE2 * sp * sp);
    return P3{(n + h) * cp * std::cos(lon * kRad), (n + h) * cp * std::sin(lon * kRad), (n * (1.0 - kE2) + h) * sp};
}

static double dist(const P3 &a, const P3 &b)
{
    return std::sqrt((a.x - b.x) * (a.x - b.x) + (a.y - b.y) * (a.y - b.y) + (a.z - b.z) * (a.z - b.z));
}

static double mod(double a, double b) { return a - b * std::floor(a / b); }

static uint32_t zones(double lat) // NL, for the latitudes used here (well inside +-87)
{
    const double a = 1.0 - std::cos(kPi / 30.0), b = std::cos(kRad * lat);
    return (uint32_t)std::floor(2.0 * kPi / std::acos(1.0 - a / (b * b)));
}

// DF17, type code tc, the altitude code with the Q bit for n x 25 - 1000 ft, the even CPR of (lat, lon)
static void position_bytes(uint8_t *b, uint32_t tc, uint32_t n, double lat, double lon)
{
    std::memset(b, 0, 14);
    const uint32_t code = (n >> 4) << 5 | 0x10u | (n & 0xFu);
    const double d_lat = 360.0 / 60.0;
    const uint32_t yz = (uint32_t)std::floor(131072.0 * mod(lat, d_lat) / d_lat + 0.5) & 0x1FFFFu;
    const double rlat = d_lat * ((double)yz / 131072.0 + std::floor(lat / d_lat));
    const double d_lon = 360.0 / (double)zones(rlat);
    const uint32_t xz = (uint32_t)std::floor(131072.0 * mod(lon, d_lon) / d_lon + 0.5) & 0x1FFFFu;
    const uint64_t me = (uint64_t)tc << 51 | (uint64_t)code << 36 | (uint64_t)yz << 17 | xz; // T = 0, F = 0 (even)
    b[0] = 0x8D;
    for (int k = 0; k < 7; ++k) b[4 + k] = (uint8_t)(me >> (48 - 8 * k));
}

struct List {
    std::vector<adsb_mlat_receiver> rcv;
    std::vector<adsb_message> msgs;
    std::vector<adsb_reception> recs;
    std::vector<adsb_wire_rx> rx;
    std::vector<double> offset, drift; // the truth
};

static List ring(uint32_t n, double radius_deg)
{
    List l;
    for (uint32_t r = 0; r < n; ++r) {
        const double az = 2.0 * kPi * r / n;
        l.rcv.push_back(adsb_mlat_receiver{47.45 + radius_deg * std::cos(az), 8.56 + 1.5 * radius_deg * std::sin(az),
                                           300.0 + 5.0 * r, 0.0});
        l.offset.push_back(r ? 1e-4 * std::sin(1.0 + r) : 0.0);
        l.drift.push_back(r ? 2e-5 * std::cos(2.0 + r) : 0.0);
    }
    return l;
}

// One message sent at time t from (lat, lon, n x 25 - 1000 ft) and heard by `heard`; 12 MHz ticks from tick_base, mod
// 2^48 in rx[] and in full in the receptions
static void add_message(List &l, double t, double lat, double lon, uint32_t alt_n, const std::vector<uint32_t> &heard,
                        uint64_t tick_base, uint32_t tc = 11)
{
    const P3 p = ecef(lat, lon, ((double)alt_n * 25.0 - 1000.0) * 0.3048);
    adsb_message m;
    std::memset(&m, 0, sizeof(m));
    position_bytes(m.bytes, tc, alt_n, lat, lon);
    m.first = (uint32_t)l.recs.size();
    m.n_receptions = (uint32_t)heard.size();
    std::vector<adsb_reception> mine;
    for (uint32_t r : heard) {
        const adsb_mlat_receiver &q = l.rcv[r];
        const double at = t + dist(p, ecef(q.latitude, q.longitude, q.height_m)) / ADSB_MLAT_C + l.offset[r] + l.drift[r] * t;
        adsb_reception e;
        e.time = tick_base + (uint64_t)std::floor(at * 12e6);
        e.frame = 0;
        e.receiver = (uint16_t)r;
        e.reserved = 0;
        mine.push_back(e);
    }
    for (size_t i = 1; i < mine.size(); ++i) // (T, j) order
        for (size_t j = i; j > 0 && mine[j].time < mine[j - 1].time; --j) std::swap(mine[j], mine[j - 1]);
    for (adsb_reception &e : mine) {
        e.frame = (uint32_t)l.rx.size();
        l.rx.push_back(adsb_wire_rx{e.time & 0xFFFFFFFFFFFFull, 0, 0, '3', e.receiver});
        l.recs.push_back(e);
    }
    m.time = mine.empty() ? 0 : mine[0].time;
    l.msgs.push_back(m);
}

struct Result {
    int rc, rc_apply;
    std::vector<adsb_clock> clocks;
    adsb_clock_header hdr;
    std::vector<adsb_reception> corrected;
    std::vector<uint8_t> state;
};

static adsb_clock_cfg cfg_of(uint32_t flags = ADSB_CLOCK_DRIFT)
{
    adsb_clock_cfg c;
    std::memset(&c, 0, sizeof(c));
    c.time_source = ADSB_MLAT_TIME_TICKS;
    c.flags = flags;
    c.seconds_per_time = 1.0 / 12e6;
    return c;
}

// Every array the mirror reads or writes is a heap block of exactly its size
static Result run(const List &l, const adsb_clock_cfg &c, size_t n_recs_told = (size_t)-1)
{
    const size_t nm = l.msgs.size(), nr = n_recs_told == (size_t)-1 ? l.recs.size() : n_recs_told, nx = l.rx.size();
    adsb_message *msgs = (adsb_message *)std::malloc(sizeof(adsb_message) * nm + 1);
    adsb_reception *recs = (adsb_reception *)std::malloc(sizeof(adsb_reception) * nr + 1);
    adsb_wire_rx *rx = (adsb_wire_rx *)std::malloc(sizeof(adsb_wire_rx) * nx + 1);
    adsb_mlat_receiver *rcv = (adsb_mlat_receiver *)std::malloc(sizeof(adsb_mlat_receiver) * l.rcv.size());
    if (nm) std::memcpy(msgs, l.msgs.data(), sizeof(adsb_message) * nm);
    if (nr) std::memcpy(recs, l.recs.data(), sizeof(adsb_reception) * nr);
    if (nx) std::memcpy(rx, l.rx.data(), sizeof(adsb_wire_rx) * nx);
    std::memcpy(rcv, l.rcv.data(), sizeof(adsb_mlat_receiver) * l.rcv.size());
    adsb_clock *clocks = (adsb_clock *)std::malloc(sizeof(adsb_clock) * l.rcv.size());
    adsb_reception *corrected = (adsb_reception *)std::malloc(sizeof(adsb_reception) * nr + 1);
    uint8_t *state = (uint8_t *)std::malloc(nr + 1);
    Result out;
    std::memset(&out.hdr, 0, sizeof(out.hdr));
    out.rc = adsb_host_clock_sync(&c, rcv, (uint32_t)l.rcv.size(), nm ? msgs : nullptr, nm, nr ? recs : nullptr, nr, rx, nx,
                                  clocks, &out.hdr, nr ? state : nullptr);
    out.rc_apply = adsb_host_clock_apply(&c, clocks, (uint32_t)l.rcv.size(), nm ? msgs : nullptr, nm, nr ? recs : nullptr,
                                         nr, rx, nx, nr ? corrected : nullptr);
    out.clocks.assign(clocks, clocks + l.rcv.size());
    out.corrected.assign(corrected, corrected + nr);
    out.state.assign(state, state + nr);
    for (void *p : {(void *)msgs, (void *)recs, (void *)rx, (void *)rcv, (void *)clocks, (void *)corrected, (void *)state})
        std::free(p);
    return out;
}

static void traffic(List &l, uint32_t n_msgs, uint64_t tick_base, uint32_t skip = 0)
{
    const uint32_t R = (uint32_t)l.rcv.size();
    for (uint32_t i = 0; i < n_msgs; ++i) {
        std::vector<uint32_t> heard;
        for (uint32_t r = 0; r < R; ++r)
            if (!skip || (r + i) % skip) heard.push_back(r);
        add_message(l, 1.0 + 0.7 * i, 47.45 + 0.6 * std::sin(0.9 * i), 8.56 + 0.9 * std::cos(1.3 * i), 400 + 37 * (i % 30), heard,
                    tick_base);
    }
}

static void check_truth(const List &l, const Result &r, double tol_s, double tol_drift)
{
    const double t0 = 1.0; // the first message's time: where tau = 0
    for (size_t u = 0; u < l.rcv.size(); ++u) {
        CHECK(std::fabs(r.clocks[u].fine_offset_s - (l.offset[u] + l.drift[u] * t0)) < tol_s);
        CHECK(std::fabs(r.clocks[u].drift - l.drift[u]) < tol_drift);
        CHECK(std::isfinite(r.clocks[u].residual_rms_s));
    }
}

int main()
{
    { // the plain case, and the same list with ticks that wrap at 2^48 inside it
        for (uint64_t base : {(uint64_t)5000000000ull, (uint64_t)((1ull << 48) - 12000000ull * 10)}) {
            List l = ring(6, 0.4);
            traffic(l, 60, base, 4);
            const Result r = run(l, cfg_of());
            CHECK(r.rc == ADSB_OK && r.rc_apply == ADSB_OK && r.hdr.flags == 0 && r.hdr.n_eligible == 60 && r.hdr.n_reached == 6);
            check_truth(l, r, 2e-7, 2e-8);
            CHECK(r.clocks[0].flags == (ADSB_CLOCK_REFERENCE | ADSB_CLOCK_REACHED));
            CHECK(r.clocks[3].flags == (ADSB_CLOCK_REACHED | ADSB_CLOCK_HAS_DRIFT));
            // corrected times of one message agree across receivers to the range differences: under 2 ms of 1 / (256 x 12e6)
            const adsb_message &m = l.msgs[7];
            for (uint32_t k = 1; k < m.n_receptions; ++k)
                CHECK(std::llabs((long long)(r.corrected[m.first + k].time - r.corrected[m.first].time)) < 2e-3 * 256 * 12e6);
        }
    }
    { // messages of 0, 1 and 2 receptions beside ordinary ones; a single message; the empty list
        List l = ring(4, 0.4);
        traffic(l, 10, 1000);
        add_message(l, 9.0, 47.5, 8.6, 500, {}, 1000);
        add_message(l, 9.5, 47.5, 8.6, 500, {2}, 1000);
        add_message(l, 10.0, 47.5, 8.6, 500, {1, 3}, 1000);
        Result r = run(l, cfg_of());
        CHECK(r.rc == ADSB_OK && r.hdr.n_messages == 13 && r.hdr.n_eligible == 11 && r.hdr.n_rows == 31);
        List one = ring(4, 0.4);
        traffic(one, 1, 1000);
        r = run(one, cfg_of());
        CHECK(r.rc == ADSB_OK && r.hdr.flags == ADSB_CLOCK_HDR_DRIFT_DROPPED && r.hdr.n_rows == 3 && r.hdr.n_reached == 4);
        for (const adsb_clock &k : r.clocks) CHECK(k.drift == 0.0 && !(k.flags & ADSB_CLOCK_HAS_DRIFT));
        List none = ring(3, 0.4);
        adsb_clock_cfg c = cfg_of();
        c.time_source = ADSB_MLAT_TIME_RECEPTION;
        c.seconds_per_tick = 1e-6;
        r = run(none, c);
        CHECK(r.rc == ADSB_OK && r.hdr.n_messages == 0 && r.hdr.n_reached == 1 && r.hdr.flags == 0);
        CHECK(r.clocks[1].flags == 0 && r.clocks[1].offset_s == 0.0);
    }
    { // stations all equal: every range difference is 0, the rows are the tick differences alone
        List l = ring(4, 0.0);
        traffic(l, 20, 1000);
        const Result r = run(l, cfg_of());
        CHECK(r.rc == ADSB_OK && r.hdr.flags == 0 && r.hdr.n_reached == 4);
        check_truth(l, r, 2e-7, 2e-8);
    }
    { // 256 receivers, two messages: 510 unknowns from 510 rows
        List l = ring(256, 0.5);
        add_message(l, 1.0, 47.5, 8.6, 600, [] { std::vector<uint32_t> v; for (uint32_t r = 0; r < 256; ++r) v.push_back(r); return v; }(), 1000);
        add_message(l, 31.0, 47.3, 8.9, 900, [] { std::vector<uint32_t> v; for (uint32_t r = 0; r < 256; ++r) v.push_back(r); return v; }(), 1000);
        const Result r = run(l, cfg_of());
        CHECK(r.rc == ADSB_OK && r.hdr.n_rows == 510 && r.hdr.n_reached == 256 && !(r.hdr.flags & ADSB_CLOCK_HDR_SINGULAR));
        for (const adsb_clock &k : r.clocks) CHECK(std::isfinite(k.offset_s) && std::isfinite(k.drift));
    }
    { // indices the lists do not have: reported, never read, the other messages still used
        List l = ring(4, 0.4);
        traffic(l, 12, 1000);
        List a = l;
        a.recs[a.msgs[5].first + 2].receiver = 4;
        Result r = run(a, cfg_of());
        CHECK(r.rc == ADSB_E_ARG && r.hdr.flags == ADSB_CLOCK_HDR_BAD_INDEX && r.hdr.n_eligible == 11 && r.hdr.n_rows == 33);
        CHECK(r.corrected[a.msgs[5].first + 2].time == a.recs[a.msgs[5].first + 2].time); // keeps its raw time
        List b = l;
        b.recs[b.msgs[7].first + 1].frame = (uint32_t)b.rx.size();
        r = run(b, cfg_of());
        CHECK(r.rc == ADSB_E_ARG && r.hdr.flags == ADSB_CLOCK_HDR_BAD_INDEX && r.hdr.n_eligible == 11);
        r = run(l, cfg_of(), l.recs.size() - 1); // the last message's receptions end past the list
        CHECK(r.rc == ADSB_E_ARG && r.hdr.flags == ADSB_CLOCK_HDR_BAD_INDEX && r.hdr.n_eligible == 11);
        List first = l;
        first.msgs[0].first = 0xFFFFFFF0u; // msgs[0], which apply takes its reference time from
        r = run(first, cfg_of());
        CHECK(r.rc == ADSB_E_ARG && r.rc_apply == ADSB_OK && r.hdr.n_eligible == 11);
    }
    { // arguments
        List l = ring(3, 0.4);
        traffic(l, 3, 1000);
        adsb_clock_cfg c = cfg_of();
        c.reference = 3;
        CHECK(run(l, c).rc == ADSB_E_ARG);
        c = cfg_of(2u);
        CHECK(run(l, c).rc == ADSB_E_ARG);
        c = cfg_of();
        c.seconds_per_time = 0.0;
        CHECK(run(l, c).rc == ADSB_E_ARG);
        c = cfg_of();
        c.max_residual_s = -1.0;
        CHECK(run(l, c).rc == ADSB_E_ARG);
        c = cfg_of();
        c.max_range_nm = std::nan("");
        CHECK(run(l, c).rc == ADSB_E_ARG);
    }
    std::printf(fails ? "clock_edges: %d FAILED\n" : "clock_edges: all passed\n", fails);
    return fails ? 1 : 0;
}
