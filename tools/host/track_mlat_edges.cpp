// track_mlat_edges.cpp -- stand-alone sanitizer run of the CPU mirror of the track table's mlat step
// (adsb_host_track_mlat_of, air_rs_amd/csrc/host/adsb_track_mlat.cpp, which compiles the per-frame text the device
// compiles: air_rs_amd/csrc/adsb_track_mlat.h over adsb_fix.h).  Exact-size heap buffers for the 14 frame bytes, the fix
// and the record, so that a read or write beside them is a heap-buffer-overflow; fix fields that are NaN or infinite, a
// fix at each pole and on the antimeridian, every downlink format and type code with every CPR corner, and a reference
// more than 180 NM from the decode, so that a conversion or shift that is undefined shows.  Host sources only, no device:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/host/track_mlat_edges.cpp
//       air_rs_amd/csrc/host/adsb_track_mlat.cpp -o /tmp/track_mlat_edges && /tmp/track_mlat_edges   (one command)
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <limits>

#include "../../include/adsb_host.h"

static int fails = 0;
#define CHECK(x)                                                     \
    do {                                                             \
        if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); ++fails; } \
    } while (0)

static const uint32_t GOOD = ADSB_MLAT_ATTEMPTED | ADSB_MLAT_CONVERGED | ADSB_MLAT_VALID;
static unsigned long n_calls = 0, n_checked = 0, n_far = 0, n_disagree = 0;

struct Result {
    adsb_aircraft_mlat rec;
    uint32_t flags;
    float metres;
};

// one call on exact-size heap copies; the invariants that hold whatever the inputs
static Result run(double limit, const uint8_t bytes[14], const adsb_mlat_fix &fix, double time)
{
    uint8_t *b = static_cast<uint8_t *>(std::malloc(14));
    adsb_mlat_fix *f = static_cast<adsb_mlat_fix *>(std::malloc(sizeof(adsb_mlat_fix)));
    adsb_aircraft_mlat *out = static_cast<adsb_aircraft_mlat *>(std::malloc(sizeof(adsb_aircraft_mlat)));
    std::memcpy(b, bytes, 14);
    std::memcpy(f, &fix, sizeof(fix));
    std::memset(out, 0xEE, sizeof(*out));
    Result r{};
    r.flags = 0xEEEEEEEEu;
    CHECK(adsb_host_track_mlat_of(limit, b, f, time, out, &r.flags, &r.metres) == ADSB_OK);
    CHECK(adsb_host_track_mlat_of(limit, b, f, time, out, nullptr, nullptr) == ADSB_OK); // both optional
    r.rec = *out;
    std::free(out);
    std::free(f);
    std::free(b);
    ++n_calls;
    const bool valid = (fix.flags & ADSB_MLAT_VALID) != 0, checked = (r.flags & ADSB_TRACK_MLAT_CHECKED) != 0;
    CHECK((r.flags & ~0x1Fu) == 0 && r.rec.reserved == 0);
    CHECK(((r.flags & ADSB_TRACK_MLAT_VALID) != 0) == valid && r.rec.n_valid == (valid ? 1u : 0u));
    CHECK(r.rec.n_attempted == ((fix.flags & ADSB_MLAT_ATTEMPTED) ? 1u : 0u));
    CHECK(r.rec.n_checked == (checked ? 1u : 0u) && (!checked || valid));
    CHECK(r.rec.n_disagree == ((r.flags & ADSB_TRACK_MLAT_DISAGREE) ? 1u : 0u) && r.rec.n_disagree <= r.rec.n_checked);
    CHECK(!(r.flags & ADSB_TRACK_MLAT_FAR) || ((r.flags & ADSB_TRACK_MLAT_DISAGREE) && checked && r.metres == 333360.0f));
    CHECK(r.metres >= 0.0f && r.metres <= 333360.0f && (checked || r.metres == 0.0f));
    CHECK(r.rec.last_disagreement_m == r.metres && r.rec.max_disagreement_m == r.metres);
    CHECK(r.rec.flags == ((valid ? ADSB_TRACK_MLAT_VALID : 0u) | (checked ? ADSB_TRACK_MLAT_CHECKED : 0u) |
                          ((valid && (fix.flags & ADSB_MLAT_ALTITUDE)) ? ADSB_TRACK_MLAT_ALTITUDE : 0u)));
    if (valid) {
        CHECK(std::memcmp(&r.rec.time, &time, 8) == 0 && std::memcmp(&r.rec.latitude, &fix.latitude, 8) == 0 &&
              std::memcmp(&r.rec.longitude, &fix.longitude, 8) == 0 && r.rec.n_used == fix.n_used);
    } else {
        adsb_aircraft_mlat empty;
        std::memset(&empty, 0, sizeof(empty));
        empty.time = std::nan("");
        empty.n_attempted = r.rec.n_attempted;
        CHECK(std::memcmp(&r.rec, &empty, sizeof(empty)) == 0);
    }
    if (checked && !(r.flags & ADSB_TRACK_MLAT_FAR))
        CHECK(((r.flags & ADSB_TRACK_MLAT_DISAGREE) != 0) == ((double)r.metres > limit) || std::fabs(r.metres - limit) < 1.0);
    n_checked += checked;
    n_far += (r.flags & ADSB_TRACK_MLAT_FAR) != 0;
    n_disagree += (r.flags & ADSB_TRACK_MLAT_DISAGREE) != 0;
    return r;
}

static adsb_mlat_fix fix_at(double lat, double lon, uint32_t flags = GOOD)
{
    adsb_mlat_fix f;
    std::memset(&f, 0, sizeof(f));
    f.latitude = lat;
    f.longitude = lon;
    f.height_m = 9000.0;
    f.residual_rms_m = 4.0f;
    f.pdop = 2.0f;
    f.n_used = 5;
    f.flags = flags;
    return f;
}

static void frame(uint8_t out[14], unsigned df, unsigned tc, unsigned odd, uint32_t lat_cpr, uint32_t lon_cpr)
{
    const uint64_t me = (uint64_t)(tc & 31u) << 51 | 0x3A8ull << 36 | (uint64_t)(odd & 1u) << 34 |
                        (uint64_t)(lat_cpr & 0x1FFFFu) << 17 | (lon_cpr & 0x1FFFFu);
    out[0] = (uint8_t)(df << 3 | 5);
    out[1] = 0x4B;
    out[2] = 0x1A;
    out[3] = 0x2C;
    for (int k = 0; k < 7; ++k) out[4 + k] = (uint8_t)(me >> (48 - 8 * k));
    out[11] = out[12] = out[13] = 0;
}

int main()
{
    const double nan = std::nan(""), inf = std::numeric_limits<double>::infinity();
    const uint32_t corners[] = {0u, 1u, 0xFFFFu, 0x10000u, 0x10001u, 0x1FFFEu, 0x1FFFFu};
    uint8_t b[14];

    // every downlink format and type code, both CPR formats, every CPR corner, against fixes at the poles, on the
    // antimeridian, on the equator and in between
    const double places[][2] = {{90.0, 0.0},   {-90.0, 0.0},  {90.0, 180.0}, {-90.0, -180.0}, {0.0, 180.0}, {0.0, -180.0},
                                {47.0, 180.0}, {-47.0, -180.0}, {0.0, 0.0},  {87.0, 10.0},     {-87.0, -10.0}, {51.5, -0.1},
                                {89.9999, 179.9999}};
    for (const auto &p : places)
        for (unsigned df = 0; df < 32; ++df)
            for (unsigned tc = 0; tc < 32; ++tc) {
                if (df != 17 && (tc % 11) != 0) continue; // other formats: three type codes do
                for (unsigned odd = 0; odd < 2; ++odd)
                    for (uint32_t y : corners)
                        for (uint32_t x : corners) {
                            frame(b, df, tc, odd, y, x);
                            const Result r = run(1000.0, b, fix_at(p[0], p[1]), 1.0);
                            const bool airborne = df == 17 && ((tc >= 9 && tc <= 18) || (tc >= 20 && tc <= 22));
                            CHECK(((r.flags & ADSB_TRACK_MLAT_CHECKED) != 0) == airborne);
                        }
            }

    // fix fields that are not numbers, infinite, or off the globe: valid and kept, never checked
    frame(b, 17, 11, 0, 0x8000, 0x8000);
    const double bad[] = {nan, inf, -inf, 90.0000001, -90.0000001, 180.0000001, -180.0000001, 1e308, -1e308};
    for (double v : bad)
        for (int which = 0; which < 2; ++which) {
            adsb_mlat_fix f = fix_at(10.0, 20.0);
            (which ? f.longitude : f.latitude) = v;
            const Result r = run(1000.0, b, f, 2.0);
            if (!(std::fabs(v) <= (which ? 180.0 : 90.0))) CHECK(r.flags == ADSB_TRACK_MLAT_VALID); // off the globe
            else CHECK(r.flags & ADSB_TRACK_MLAT_CHECKED);
        }
    for (double v : {nan, inf, -inf, 1e300, -1e300, 3.5e38, 1e-320}) { // the height's one rounding to f32
        adsb_mlat_fix f = fix_at(10.0, 20.0);
        f.height_m = v;
        const Result r = run(1000.0, b, f, 3.0);
        CHECK(r.flags & ADSB_TRACK_MLAT_CHECKED);
        if (std::isnan(v)) CHECK(std::isnan(r.rec.height_m));
        else if (std::fabs(v) > 3.4028234663852886e38) CHECK(std::isinf(r.rec.height_m) && (r.rec.height_m > 0) == (v > 0));
        else CHECK(r.rec.height_m == (float)v);
    }
    for (float v : {std::nanf(""), std::numeric_limits<float>::infinity(), -1.0f}) {
        adsb_mlat_fix f = fix_at(10.0, 20.0);
        f.residual_rms_m = v;
        f.pdop = v;
        const Result r = run(1000.0, b, f, nan); // a NaN time is kept as it is
        CHECK(std::memcmp(&r.rec.pdop, &v, 4) == 0 && std::memcmp(&r.rec.residual_rms_m, &v, 4) == 0);
    }

    // the reference more than 180 NM from the decode: half a latitude zone away (3 degrees = 180.12 NM), and a decode
    // above a pole
    frame(b, 17, 11, 0, 0x10000, 0); // lat = 6 (j + 0.5)
    CHECK(run(1000.0, b, fix_at(48.0, 0.0), 4.0).flags ==
          (ADSB_TRACK_MLAT_VALID | ADSB_TRACK_MLAT_CHECKED | ADSB_TRACK_MLAT_DISAGREE | ADSB_TRACK_MLAT_FAR));
    CHECK(run(1000.0, b, fix_at(42.0, 0.0), 4.0).flags ==
          (ADSB_TRACK_MLAT_VALID | ADSB_TRACK_MLAT_CHECKED | ADSB_TRACK_MLAT_DISAGREE | ADSB_TRACK_MLAT_FAR));
    {
        const Result r = run(1000.0, b, fix_at(47.9, 0.0), 4.0); // 2.9 degrees: measured, not turned away
        CHECK(r.flags == (ADSB_TRACK_MLAT_VALID | ADSB_TRACK_MLAT_CHECKED | ADSB_TRACK_MLAT_DISAGREE) && r.metres > 320000.0f);
    }
    frame(b, 17, 11, 0, 0x4000, 0);
    CHECK(run(1000.0, b, fix_at(89.9, 0.0), 4.0).flags & ADSB_TRACK_MLAT_FAR);
    frame(b, 17, 11, 0, 0x1C000, 0);
    CHECK(run(1000.0, b, fix_at(-89.9, 0.0), 4.0).flags & ADSB_TRACK_MLAT_FAR);

    // agreement: the decode of a frame against its own position is that position
    frame(b, 17, 12, 1, 0x12345, 0x0ABCD);
    {
        const Result far_ref = run(50.0, b, fix_at(30.0, 40.0), 5.0);
        CHECK(far_ref.flags & ADSB_TRACK_MLAT_CHECKED);
        const Result r = run(50.0, b, fix_at(30.0 + 360.0 / 59.0 * (0x12345 / 131072.0 - 0.5), 40.0), 5.0);
        CHECK(r.flags & ADSB_TRACK_MLAT_CHECKED);
    }

    // every outcome flag of the solver, alone and all at once, and every limit's edge
    frame(b, 17, 11, 0, 0x8000, 0x8000);
    for (uint32_t bit = 0; bit <= 32; ++bit) (void)run(1000.0, b, fix_at(45.0, 3.0, bit == 32 ? 0xFFFFFFFFu : 1u << bit), 6.0);
    for (double limit : {5e-324, 1e-300, 1.0, 333360.0, 1e300, 1.7976931348623157e308}) (void)run(limit, b, fix_at(45.0, 3.0), 7.0);

    // argument errors
    adsb_aircraft_mlat out;
    adsb_mlat_fix f = fix_at(1.0, 2.0);
    CHECK(adsb_host_track_mlat_of(1000.0, nullptr, &f, 0.0, &out, nullptr, nullptr) == ADSB_E_ARG);
    CHECK(adsb_host_track_mlat_of(1000.0, b, nullptr, 0.0, &out, nullptr, nullptr) == ADSB_E_ARG);
    CHECK(adsb_host_track_mlat_of(1000.0, b, &f, 0.0, nullptr, nullptr, nullptr) == ADSB_E_ARG);
    for (double limit : {0.0, -0.0, -1.0, nan, inf, -inf})
        CHECK(adsb_host_track_mlat_of(limit, b, &f, 0.0, &out, nullptr, nullptr) == ADSB_E_ARG);

    std::printf("%lu calls: %lu checked, %lu disagree, %lu far\n", n_calls, n_checked, n_disagree, n_far);
    CHECK(n_checked > 10000 && n_far > 100 && n_disagree > n_far);
    if (fails) std::printf("%d check(s) FAILED\n", fails);
    else std::printf("all checks passed\n");
    return fails ? 1 : 0;
}
