// track_filter_edges.cpp -- stand-alone sanitizer run of the CPU mirror of the track table's filter
// (adsb_host_track_filter_operand / _step, air_rs_amd/csrc/host/adsb_track_filter.cpp, which compiles the text the device
// compiles: air_rs_amd/csrc/adsb_track_filter.h).  Exact-size heap buffers for the fix, the operand, the record and the
// per-frame output, so a read or write past any of them is caught; hostile values in every field the text reads.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/host/track_filter_edges.cpp
//       air_rs_amd/csrc/host/adsb_track_filter.cpp -o /tmp/track_filter_edges && /tmp/track_filter_edges   (one command)
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>

#include "../../include/adsb_host.h"

#define CHECK(x)                                                     \
    do {                                                             \
        if (!(x)) {                                                  \
            std::printf("FAILED line %d: %s\n", __LINE__, #x);       \
            std::exit(1);                                            \
        }                                                            \
    } while (0)

int main()
{
    const double inf = std::numeric_limits<double>::infinity(), nan = std::nan("");
    const double lats[] = {47.0, 89.0, 89.0000001, -89.0, -90.0, 0.0, nan, inf, -inf, 1e300};
    const double lons[] = {8.0, 180.0, -180.0, 179.9999, -179.9999, 540.0, nan, inf, 1e300};
    const double heights[] = {10000.0, -1000.0, -1000.001, 100000.0, 100000.001, nan, inf, -inf};
    const float dops[] = {1.0f, 20.0f, 20.5f, 50.0f, 50.5f, 0.0f, -1.0f, 1e-38f, 3e38f, (float)nan, (float)inf};
    const float residuals[] = {3.0f, 30.0f, 60.0f, 0.0f, -5.0f, 3e38f, (float)nan, (float)inf};
    const uint32_t flag_sets[] = {0x103u, 0x107u, 0x1u, 0x0u, 0x21u, 0xFFFFFFFFu};
    adsb_track_filter_cfg cfgs[4];
    std::memset(cfgs, 0, sizeof(cfgs));
    cfgs[1].max_outliers = 1, cfgs[1].min_run = 1, cfgs[1].gate = 0.5;
    cfgs[2].accel_h = 1e-300, cfgs[2].accel_v = 1e300, cfgs[2].reset_gap_s = 1e-9, cfgs[2].range_sigma_m = 1e150;
    cfgs[3].max_hdop = 1e30, cfgs[3].max_vdop = 1e30, cfgs[3].init_speed_sigma_h = 1e150, cfgs[3].max_outliers = 0xFFFFFFFFu;
    unsigned long long calls = 0, usable = 0, applied = 0, outliers = 0, skipped = 0, resets = 0;
    for (const adsb_track_filter_cfg &cfg : cfgs) {
        std::unique_ptr<adsb_aircraft_filter> rec(new adsb_aircraft_filter);
        std::memset(rec.get(), 0, sizeof(*rec));
        rec->time = nan;
        unsigned step = 0;
        for (double lat : lats)
            for (double lon : lons)
                for (double h : heights)
                    for (float hdop : dops)
                        for (float res : residuals) {
                            std::unique_ptr<adsb_mlat_fix> fix(new adsb_mlat_fix);
                            std::unique_ptr<adsb_filter_operand> op(new adsb_filter_operand);
                            std::unique_ptr<adsb_frame_filter> out(new adsb_frame_filter);
                            std::memset(fix.get(), 0, sizeof(*fix));
                            fix->latitude = lat + (step % 5 == 2 ? 3.0 : 0.0), fix->longitude = lon, fix->height_m = h; // now and then 330 km off
                            fix->hdop = hdop, fix->vdop = dops[step % 11], fix->residual_rms_m = res;
                            fix->flags = flag_sets[step % 6];
                            // mostly forward in half seconds; now and then back, NaN, equal, or past the reset gap
                            double t = 0.5 * step + (step % 101 == 0 ? 100.0 : 0.0);
                            if (step % 10 == 3) t -= 3.0;
                            if (step % 37 == 5) t = nan;
                            if (step % 13 == 7) t = 0.5 * (step - 1);
                            ++step;
                            CHECK(adsb_host_track_filter_operand(&cfg, fix.get(), t, step % 7 != 0, op.get()) == ADSB_OK);
                            const adsb_aircraft_filter before = *rec;
                            CHECK(adsb_host_track_filter_step(&cfg, rec.get(), op.get(), out.get()) == ADSB_OK);
                            ++calls;
                            if (!(op->flags & ADSB_TRACK_FILTER_USABLE)) { // 64 zero bytes, and nothing moves
                                const adsb_filter_operand zero{};
                                const adsb_frame_filter none{};
                                CHECK(!std::memcmp(op.get(), &zero, sizeof(zero)) && !std::memcmp(out.get(), &none, sizeof(none)));
                                CHECK(!std::memcmp(rec.get(), &before, sizeof(before)));
                                continue;
                            }
                            ++usable;
                            CHECK(std::fabs(op->latitude) <= 89.0 && op->rn > 0.0 && op->re > 0.0 && op->var_h > 0.0);
                            CHECK(std::isfinite(op->var_h) && std::isfinite(op->var_v) && std::isfinite(op->longitude));
                            CHECK((out->flags & ADSB_TRACK_FILTER_USABLE) && (rec->flags & ADSB_TRACK_FILTER_RUNNING));
                            CHECK(!(rec->flags & ~7u) && out->reserved == 0);
                            applied += (out->flags & ADSB_TRACK_FILTER_APPLIED) != 0;
                            outliers += (out->flags & ADSB_TRACK_FILTER_OUTLIER) != 0;
                            skipped += (out->flags & ADSB_TRACK_FILTER_SKIPPED) != 0;
                            resets += (out->flags & ADSB_TRACK_FILTER_RESET) != 0;
                            if (out->flags & ADSB_TRACK_FILTER_INIT) CHECK(rec->run == 1 && rec->latitude == op->latitude);
                            if (out->flags & ADSB_TRACK_FILTER_SKIPPED) CHECK(rec->n_skipped == before.n_skipped + 1);
                            for (unsigned k = 0; k < 8; ++k) CHECK(rec->reserved[k] == 0);
                        }
    }
    {   // an infinite frame time: a restart, and every later frame of a finite time is skipped
        adsb_mlat_fix fix{};
        fix.latitude = 47.0, fix.longitude = 8.0, fix.height_m = 9000.0, fix.hdop = 1.0f, fix.vdop = 2.0f, fix.flags = 0x103u;
        adsb_aircraft_filter rec{};
        rec.time = nan;
        adsb_filter_operand op;
        adsb_frame_filter out;
        const double ts[] = {1.0, 2.0, inf, 3.0, inf, 1e300};
        const uint32_t want[] = {0x500u, 0x300u, 0xD00u, 0x2100u, 0x2100u, 0x2100u}; // inf - inf is NaN: skipped
        for (int k = 0; k < 6; ++k) {
            CHECK(adsb_host_track_filter_operand(nullptr, &fix, ts[k], 1, &op) == ADSB_OK);
            CHECK(adsb_host_track_filter_step(nullptr, &rec, &op, &out) == ADSB_OK);
            CHECK(out.flags == want[k]);
        }
    }
    adsb_track_filter_cfg bad{};
    bad.gate = -1.0;
    adsb_mlat_fix f{};
    adsb_filter_operand o{};
    adsb_aircraft_filter a{};
    CHECK(adsb_host_track_filter_operand(&bad, &f, 0.0, 1, &o) == ADSB_E_ARG);
    CHECK(adsb_host_track_filter_step(&bad, &a, &o, nullptr) == ADSB_E_ARG);
    CHECK(adsb_host_track_filter_operand(nullptr, nullptr, 0.0, 1, &o) == ADSB_E_ARG);
    CHECK(adsb_host_track_filter_step(nullptr, &a, &o, nullptr) == ADSB_OK);
    std::printf("%llu calls: %llu usable, %llu applied, %llu outliers, %llu skipped, %llu restarts\nall checks passed\n", calls,
                usable, applied, outliers, skipped, resets);
    return 0;
}
