// mlat_edges.cpp -- stand-alone sanitizer run of the CPU mirror of multilaterate (adsb_host_multilaterate,
// air_rs_amd/csrc/host/adsb_mlat.cpp over air_rs_amd/csrc/adsb_mlat.h, the text the device compiles too).  Exact-size heap
// buffers, so that one fix past fixes[n_msgs] or one reception read past recs[n_recs] is a heap-buffer-overflow; messages
// of 0, 3, 256 and 257 receptions; the same receiver twice; stations all equal and collinear (no division by zero, no
// NaN in a flag decision, SINGULAR where the geometry has no solution); ticks that wrap at 2^48; indices the lists do not
// have (receiver, reception range, frame), which must be reported and never read; the empty list.  Every result is
// checked against what the definition says.  Host sources only, no device:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/host/mlat_edges.cpp air_rs_amd/csrc/host/adsb_mlat.cpp -o /tmp/mlat_edges && /tmp/mlat_edges
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

static const double kA = 6378137.0, kE2 = 6.69437999014e-3, kRad = 3.14159265358979323846 / 180.0;

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

// DF17, type code 11, altitude code with the Q bit for n x 25 - 1000 ft (the parity bytes do not matter here)
static void position_bytes(uint8_t *b, uint32_t n)
{
    std::memset(b, 0, 14);
    const uint32_t code = (n >> 4) << 5 | 0x10u | (n & 0xFu);
    b[0] = 0x8D;
    b[4] = 11u << 3;
    b[5] = (uint8_t)(code >> 4);
    b[6] = (uint8_t)((code & 0xFu) << 4);
}

struct List {
    std::vector<adsb_mlat_receiver> rcv;
    std::vector<adsb_message> msgs;
    std::vector<adsb_reception> recs;
    std::vector<adsb_wire_rx> rx;
};

// One message from an emitter at (lat, lon, h) heard by the receivers in `heard` (repeats allowed: a later reception
// 40 ticks behind), ticks of `spt` seconds from tick_base, mod 2^48 in rx[]
static void add_message(List &l, double lat, double lon, uint32_t alt_n, const std::vector<uint32_t> &heard, double spt,
                        uint64_t tick_base)
{
    const P3 p = ecef(lat, lon, ((double)alt_n * 25.0 - 1000.0) * 0.3048);
    adsb_message m;
    std::memset(&m, 0, sizeof(m));
    position_bytes(m.bytes, alt_n);
    m.first = (uint32_t)l.recs.size();
    m.n_receptions = (uint32_t)heard.size();
    std::vector<adsb_reception> mine;
    std::vector<int> seen(l.rcv.size(), 0);
    for (uint32_t r : heard) {
        const adsb_mlat_receiver &q = l.rcv[r];
        const double t = dist(p, ecef(q.latitude, q.longitude, q.height_m)) / ADSB_MLAT_C + q.clock_offset_s;
        adsb_reception e;
        e.time = tick_base + (uint64_t)std::floor(t / spt) + 40u * (uint64_t)seen[r]++;
        e.frame = 0;
        e.receiver = (uint16_t)r;
        e.reserved = 0;
        mine.push_back(e);
    }
    for (size_t a = 1; a < mine.size(); ++a) // (T, j) order
        for (size_t b = a; b > 0 && mine[b].time < mine[b - 1].time; --b) std::swap(mine[b], mine[b - 1]);
    for (adsb_reception &e : mine) {
        e.frame = (uint32_t)l.rx.size();
        adsb_wire_rx x;
        std::memset(&x, 0, sizeof(x));
        x.ticks = e.time & 0xFFFFFFFFFFFFull;
        x.receiver = e.receiver;
        l.rx.push_back(x);
        l.recs.push_back(e);
    }
    if (!mine.empty()) m.time = mine[0].time;
    l.msgs.push_back(m);
}

static std::vector<adsb_mlat_receiver> ring(uint32_t n)
{
    std::vector<adsb_mlat_receiver> r(n);
    for (uint32_t k = 0; k < n; ++k) {
        const double az = 2.0 * 3.14159265358979323846 * (k + 0.3 * ((k * 7) % 3)) / n, rad = 0.35 + 0.2 * ((k * 5) % 7) / 7.0;
        r[k] = adsb_mlat_receiver{47.45 + rad * std::cos(az), 8.56 + 1.5 * rad * std::sin(az), 300.0 + 1500.0 * ((k * 3) % 11) / 11.0, 0.0};
    }
    return r;
}

// exact-size heap copies of everything the mirror reads or writes
static int run(const List &l, adsb_mlat_cfg cfg, std::vector<adsb_mlat_fix> &out, adsb_mlat_header &h, size_t n_recs_given,
               size_t n_rx_given, uint32_t n_receivers_given)
{
    const auto copy = [](const void *src, size_t bytes) {
        void *p = std::malloc(bytes ? bytes : 1);
        if (bytes) std::memcpy(p, src, bytes);
        return p;
    };
    adsb_mlat_receiver *rcv = (adsb_mlat_receiver *)copy(l.rcv.data(), sizeof(adsb_mlat_receiver) * n_receivers_given);
    adsb_message *msgs = (adsb_message *)copy(l.msgs.data(), sizeof(adsb_message) * l.msgs.size());
    adsb_reception *recs = (adsb_reception *)copy(l.recs.data(), sizeof(adsb_reception) * n_recs_given);
    adsb_wire_rx *rx = (adsb_wire_rx *)copy(l.rx.data(), sizeof(adsb_wire_rx) * n_rx_given);
    adsb_mlat_fix *fixes = (adsb_mlat_fix *)std::malloc(l.msgs.size() ? sizeof(adsb_mlat_fix) * l.msgs.size() : 1);
    const int rc = adsb_host_multilaterate(&cfg, rcv, n_receivers_given, l.msgs.empty() ? nullptr : msgs, l.msgs.size(),
                                           n_recs_given ? recs : nullptr, n_recs_given, n_rx_given ? rx : nullptr, n_rx_given,
                                           l.msgs.empty() ? nullptr : fixes, &h);
    out.assign(fixes, fixes + l.msgs.size());
    std::free(rcv);
    std::free(msgs);
    std::free(recs);
    std::free(rx);
    std::free(fixes);
    return rc;
}

static int run(const List &l, const adsb_mlat_cfg &cfg, std::vector<adsb_mlat_fix> &out, adsb_mlat_header &h)
{
    return run(l, cfg, out, h, l.recs.size(), l.rx.size(), (uint32_t)l.rcv.size());
}

static adsb_mlat_cfg cfg_of(uint32_t source, double spt, uint32_t flags)
{
    adsb_mlat_cfg c;
    std::memset(&c, 0, sizeof(c));
    c.time_source = source;
    c.flags = flags;
    c.seconds_per_tick = spt;
    return c;
}

static bool finite_fix(const adsb_mlat_fix &f)
{
    return std::isfinite(f.latitude) && std::isfinite(f.longitude) && std::isfinite(f.height_m) && std::isfinite(f.time_s) &&
           std::isfinite(f.residual_rms_m) && std::isfinite(f.pdop) && std::isfinite(f.hdop) && std::isfinite(f.vdop);
}

int main()
{
    std::vector<adsb_mlat_fix> fx;
    adsb_mlat_header h;
    const double ns = 1e-9;

    { // counts of 0, 3, 256 and 257 receptions, and a repeated receiver, in one list of 256 receivers
        List l;
        l.rcv = ring(256);
        std::vector<uint32_t> all(256), over, three = {7, 90, 200}, twice = {1, 50, 100, 150, 200, 250, 100};
        for (uint32_t r = 0; r < 256; ++r) all[r] = r;
        over = all;
        over.push_back(17);
        add_message(l, 47.9, 9.3, 1400, {}, ns, 1000);
        add_message(l, 47.9, 9.3, 1400, three, ns, 2000000);
        add_message(l, 47.1, 8.1, 1000, all, ns, 4000000);
        add_message(l, 47.1, 8.1, 1000, over, ns, 6000000);
        add_message(l, 47.6, 8.9, 800, twice, ns, 8000000);
        CHECK(run(l, cfg_of(ADSB_MLAT_TIME_RECEPTION, ns, 0), fx, h) == ADSB_OK);
        CHECK(fx[0].flags == ADSB_MLAT_TOO_FEW && fx[0].n_used == 0);
        CHECK(fx[1].flags == ADSB_MLAT_TOO_FEW && fx[1].n_used == 3 && fx[1].latitude == 0.0);
        CHECK((fx[2].flags & ADSB_MLAT_VALID) && fx[2].n_used == 256);
        CHECK(std::fabs(fx[2].latitude - 47.1) < 1e-3 && std::fabs(fx[2].longitude - 8.1) < 1e-3);
        CHECK(fx[3].flags == ADSB_MLAT_TOO_MANY && fx[3].n_used == 0);
        CHECK((fx[4].flags & ADSB_MLAT_ATTEMPTED) && fx[4].n_used == 6); // the later reception of receiver 100 is not used
        CHECK(std::fabs(fx[4].latitude - 47.6) < 1e-2 && std::fabs(fx[4].longitude - 8.9) < 1e-2);
        CHECK(h.n_messages == 5 && h.n_attempted == 2 && h.n_valid >= 1 && h.flags == 0);
        CHECK(run(l, cfg_of(ADSB_MLAT_TIME_RECEPTION, ns, ADSB_MLAT_USE_ALTITUDE), fx, h) == ADSB_OK);
        CHECK((fx[1].flags & (ADSB_MLAT_ATTEMPTED | ADSB_MLAT_ALTITUDE)) == (ADSB_MLAT_ATTEMPTED | ADSB_MLAT_ALTITUDE));
        CHECK(h.n_attempted == 3);
        for (const adsb_mlat_fix &f : fx) CHECK(finite_fix(f));
        std::printf("counts 0 / 3 / 256 / 257 and a repeated receiver: checked\n");
    }
    { // degenerate stations
        List l;
        l.rcv = ring(6);
        for (adsb_mlat_receiver &r : l.rcv) r = l.rcv[0];
        add_message(l, 47.9, 9.3, 1400, {0, 1, 2, 3, 4, 5}, ns, 1000);
        for (uint32_t flags : {0u, (uint32_t)ADSB_MLAT_USE_ALTITUDE}) {
            CHECK(run(l, cfg_of(ADSB_MLAT_TIME_RECEPTION, ns, flags), fx, h) == ADSB_OK);
            CHECK((fx[0].flags & ADSB_MLAT_SINGULAR) && !(fx[0].flags & ADSB_MLAT_VALID) && fx[0].pdop == 0.0f && finite_fix(fx[0]));
        }
        List c;
        c.rcv = ring(6);
        for (uint32_t k = 0; k < 6; ++k) c.rcv[k] = adsb_mlat_receiver{47.0 + 0.1 * k, 8.0, 500.0, 0.0};
        add_message(c, 47.9, 9.3, 1400, {0, 1, 2, 3, 4, 5}, ns, 1000);
        add_message(c, 47.2, 8.0, 1400, {0, 1, 2, 3, 4, 5}, ns, 5000000); // on the line itself
        for (uint32_t flags : {0u, (uint32_t)ADSB_MLAT_USE_ALTITUDE}) {
            CHECK(run(c, cfg_of(ADSB_MLAT_TIME_RECEPTION, ns, flags), fx, h) == ADSB_OK);
            for (const adsb_mlat_fix &f : fx) CHECK((f.flags & ADSB_MLAT_ATTEMPTED) && finite_fix(f));
        }
        // an emitter standing on a station: |p - s| = 0 on the way is not divided by
        List z;
        z.rcv = ring(5);
        add_message(z, z.rcv[2].latitude, z.rcv[2].longitude, (uint32_t)((z.rcv[2].height_m / 0.3048 + 1000.0) / 25.0), {0, 1, 2, 3, 4}, ns, 1000);
        CHECK(run(z, cfg_of(ADSB_MLAT_TIME_RECEPTION, ns, ADSB_MLAT_USE_ALTITUDE), fx, h) == ADSB_OK && finite_fix(fx[0]));
        std::printf("stations all equal (SINGULAR), collinear, emitter on a station: checked\n");
    }
    { // tick wrap: the same fixes from ticks that cross 2^48 as from ticks that do not
        List a, b;
        a.rcv = b.rcv = ring(6);
        const double tick = 1.0 / 12e6;
        for (int k = 0; k < 4; ++k) {
            add_message(a, 47.2 + 0.2 * k, 8.2 + 0.3 * k, 1200, {0, 1, 2, 3, 4, 5}, tick, 5000);
            add_message(b, 47.2 + 0.2 * k, 8.2 + 0.3 * k, 1200, {0, 1, 2, 3, 4, 5}, tick, (1ull << 48) - 3000);
        }
        std::vector<adsb_mlat_fix> fa, fb;
        CHECK(run(a, cfg_of(ADSB_MLAT_TIME_TICKS, 0.0, 0), fa, h) == ADSB_OK);
        CHECK(run(b, cfg_of(ADSB_MLAT_TIME_TICKS, 0.0, 0), fb, h) == ADSB_OK);
        bool wrapped = false;
        for (const adsb_wire_rx &x : b.rx) wrapped = wrapped || x.ticks < 100000;
        CHECK(wrapped && h.n_valid == 4);
        CHECK(std::memcmp(fa.data(), fb.data(), sizeof(adsb_mlat_fix) * fa.size()) == 0);
        std::printf("tick wrap at 2^48: the same bytes\n");
    }
    { // indices the lists do not have: reported, never read (the exact-size buffers end right behind the valid part)
        List l;
        l.rcv = ring(6);
        add_message(l, 47.9, 9.3, 1400, {0, 1, 2, 3, 4}, ns, 1000);
        add_message(l, 47.3, 8.3, 1400, {0, 1, 2, 3, 5}, ns, 3000000);
        CHECK(run(l, cfg_of(ADSB_MLAT_TIME_RECEPTION, ns, 0), fx, h, l.recs.size(), 0, 5) == ADSB_E_ARG);
        CHECK((fx[0].flags & ADSB_MLAT_VALID) && fx[1].flags == ADSB_MLAT_BAD_INDEX && h.flags == ADSB_MLAT_HDR_BAD_INDEX);
        CHECK(run(l, cfg_of(ADSB_MLAT_TIME_RECEPTION, ns, 0), fx, h, l.recs.size() - 1, 0, 6) == ADSB_E_ARG);
        CHECK((fx[0].flags & ADSB_MLAT_VALID) && fx[1].flags == ADSB_MLAT_BAD_INDEX);
        CHECK(run(l, cfg_of(ADSB_MLAT_TIME_TICKS, ns, 0), fx, h, l.recs.size(), l.rx.size() - 1, 6) == ADSB_E_ARG);
        CHECK((fx[0].flags & ADSB_MLAT_VALID) && fx[1].flags == ADSB_MLAT_BAD_INDEX);
        l.msgs[1].first = 0xFFFFFFFFu; // first + n wraps in 32 bits, not in the check
        CHECK(run(l, cfg_of(ADSB_MLAT_TIME_RECEPTION, ns, 0), fx, h) == ADSB_E_ARG && fx[1].flags == ADSB_MLAT_BAD_INDEX);
        List none;
        none.rcv = ring(4);
        CHECK(run(none, cfg_of(ADSB_MLAT_TIME_RECEPTION, ns, 0), fx, h) == ADSB_OK && h.n_messages == 0 && h.n_valid == 0);
        std::printf("bad receiver / reception range / frame index, the empty list: checked\n");
    }
    std::printf(fails ? "mlat_edges: %d FAILED\n" : "mlat_edges: all checks passed\n", fails);
    return fails ? 1 : 0;
}
