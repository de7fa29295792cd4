// track_modes_edges.cpp -- stand-alone sanitizer run of the CPU mirror of the track table's Mode S step
// (adsb_host_track_modes_of and adsb_host_track_modes_merge, air_rs_amd/csrc/host/adsb_track_modes.cpp, which compiles
// the text the device compiles: air_rs_amd/csrc/adsb_track_modes.h).  Exact-size heap buffers for the record in and the
// records out, so that a read or write beside them is a heap-buffer-overflow; every DF 0..255 with every kind 0..255's
// low values and every flags word, extreme altitudes and squawks, callsigns without a terminator, NaN and infinite
// times, counts at 2^32 - 2 and 2^32 - 1, and folds in both groupings.  Host sources only, no device:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/host/track_modes_edges.cpp
//       air_rs_amd/csrc/host/adsb_track_modes.cpp -o /tmp/track_modes_edges && /tmp/track_modes_edges   (one command)
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

static unsigned long n_calls = 0, n_accepted = 0, n_merges = 0;

static bool same_bytes(const adsb_aircraft_modes &a, const adsb_aircraft_modes &b) { return std::memcmp(&a, &b, sizeof(a)) == 0; }

static bool is_empty(const adsb_aircraft_modes &a)
{
    adsb_aircraft_modes z = a;
    if (!std::isnan(a.altitude_time) || !std::isnan(a.squawk_time) || !std::isnan(a.callsign_time)) return false;
    z.altitude_time = z.squawk_time = z.callsign_time = 0.0;
    static const unsigned char zeros[sizeof(adsb_aircraft_modes)] = {};
    return std::memcmp(&z, zeros, sizeof(z)) == 0;
}

// one call on exact-size heap copies; the invariants that hold whatever the inputs
static adsb_aircraft_modes one(const adsb_modes_rec &rec, double time)
{
    adsb_modes_rec *r = static_cast<adsb_modes_rec *>(std::malloc(sizeof(adsb_modes_rec)));
    adsb_aircraft_modes *out = static_cast<adsb_aircraft_modes *>(std::malloc(sizeof(adsb_aircraft_modes)));
    std::memcpy(r, &rec, sizeof(rec));
    std::memset(out, 0xEE, sizeof(*out));
    uint32_t ok = 0xEEEEEEEEu;
    CHECK(adsb_host_track_modes_of(r, time, out, &ok) == ADSB_OK);
    CHECK(adsb_host_track_modes_of(r, time, out, nullptr) == ADSB_OK); // optional
    const adsb_aircraft_modes a = *out;
    std::free(out);
    std::free(r);
    ++n_calls;
    const bool accepted = rec.kind == ADSB_MODES_SELF || rec.kind == ADSB_MODES_KNOWN;
    CHECK(ok == (accepted ? 1u : 0u));
    for (int k = 0; k < 6; ++k) CHECK(a.reserved[k] == 0);
    if (!accepted) {
        CHECK(is_empty(a));
        return a;
    }
    ++n_accepted;
    const bool squitter = rec.df == 17 || rec.df == 18;
    const bool surv = rec.df == 4 || rec.df == 5 || rec.df == 20 || rec.df == 21, air = rec.df == 0 || rec.df == 16;
    CHECK(((a.flags & ADSB_TRACK_MODES_SQUITTER) != 0) == squitter && a.n_replies == (squitter ? 0u : 1u));
    CHECK(a.n_allcall == (rec.df == 11 ? 1u : 0u) && a.n_surveillance == (surv ? 1u : 0u) && a.n_airair == (air ? 1u : 0u));
    CHECK(a.last_df == rec.df);
    CHECK(((a.flags & ADSB_TRACK_MODES_ALT) != 0) == ((rec.flags & ADSB_MODES_ALT) != 0));
    CHECK((a.flags & ADSB_TRACK_MODES_ALT) ? (a.altitude_ft == rec.altitude_ft && std::memcmp(&a.altitude_time, &time, 8) == 0)
                                           : (a.altitude_ft == 0 && std::isnan(a.altitude_time)));
    CHECK((a.flags & ADSB_TRACK_MODES_SQUAWK) ? (a.squawk == rec.squawk && std::memcmp(&a.squawk_time, &time, 8) == 0)
                                              : (a.squawk == 0 && std::isnan(a.squawk_time)));
    CHECK((a.flags & ADSB_TRACK_MODES_CALLSIGN) ? (std::memcmp(a.callsign, rec.callsign, 8) == 0 && std::memcmp(&a.callsign_time, &time, 8) == 0)
                                                : (a.callsign[0] == 0 && std::isnan(a.callsign_time)));
    CHECK(((a.flags & ADSB_TRACK_MODES_STATUS) != 0) == surv && a.fs == (surv ? rec.fs : 0));
    CHECK((a.flags & (ADSB_TRACK_MODES_ALERT | ADSB_TRACK_MODES_SPI)) == (surv ? (rec.flags & (ADSB_MODES_ALERT | ADSB_MODES_SPI)) : 0));
    CHECK((a.flags & ADSB_TRACK_MODES_GROUND) == ((surv || air) ? (rec.flags & ADSB_MODES_GROUND) : 0));
    CHECK((a.flags & ~0x37Du) == 0);
    return a;
}

static adsb_aircraft_modes merge(const adsb_aircraft_modes &into, const adsb_aircraft_modes &later)
{
    adsb_aircraft_modes *a = static_cast<adsb_aircraft_modes *>(std::malloc(sizeof(adsb_aircraft_modes)));
    adsb_aircraft_modes *b = static_cast<adsb_aircraft_modes *>(std::malloc(sizeof(adsb_aircraft_modes)));
    std::memcpy(a, &into, sizeof(into));
    std::memcpy(b, &later, sizeof(later));
    CHECK(adsb_host_track_modes_merge(a, b) == ADSB_OK);
    CHECK(same_bytes(*b, later)); // the later record is read only
    const adsb_aircraft_modes o = *a;
    std::free(b);
    std::free(a);
    ++n_merges;
    return o;
}

int main()
{
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const double times[] = {0.0, -0.0, 1.5, 1e300, -1e300, 5e-324, inf, -inf, nan};
    adsb_modes_rec rec;
    adsb_aircraft_modes empty;
    {
        std::memset(&rec, 0, sizeof(rec));
        rec.kind = ADSB_MODES_PARITY;
        empty = one(rec, 0.0);
        CHECK(is_empty(empty));
    }
    CHECK(adsb_host_track_modes_of(nullptr, 0.0, &empty, nullptr) == ADSB_E_ARG);
    CHECK(adsb_host_track_modes_of(&rec, 0.0, nullptr, nullptr) == ADSB_E_ARG);
    CHECK(adsb_host_track_modes_merge(nullptr, &empty) == ADSB_E_ARG && adsb_host_track_modes_merge(&empty, nullptr) == ADSB_E_ARG);

    // every DF byte x kinds 0..7 and 255 x every flags bit pattern of the low 8 bits, and the unused high bits set
    static adsb_aircraft_modes kept[4096];
    unsigned n_kept = 0;
    for (unsigned df = 0; df < 256; ++df)
        for (unsigned kind : {0u, 1u, 2u, 3u, 4u, 5u, 7u, 255u})
            for (unsigned flags = 0; flags < 256; ++flags) {
                std::memset(&rec, 0xA5, sizeof(rec)); // reserved and unused fields are not zero
                rec.df = (uint8_t)df;
                rec.kind = (uint8_t)kind;
                rec.flags = (uint16_t)(flags | ((df & 1) ? 0xFF00u : 0u));
                rec.address = df * 0x010101u + (kind << 24);
                rec.altitude_ft = (df & 2) ? std::numeric_limits<int32_t>::min() : std::numeric_limits<int32_t>::max();
                rec.squawk = (uint16_t)(0xFFFFu - df);
                rec.fs = (uint8_t)(df ^ 0xFF);
                std::memcpy(rec.callsign, "NOTERMIN", 8); // eight characters, no NUL
                const adsb_aircraft_modes a = one(rec, times[(df + flags) % 9]);
                if (kind <= 1 && n_kept < 4096 && (df < 32 || df % 16 == 1) && flags % 5 == 0) kept[n_kept++] = a;
            }
    CHECK(n_kept > 1000);

    // the empty record is the identity; folds in both groupings agree
    for (unsigned k = 0; k < n_kept; ++k) {
        CHECK(same_bytes(merge(empty, kept[k]), kept[k]));
        CHECK(same_bytes(merge(kept[k], empty), kept[k]));
    }
    for (unsigned k = 0; k + 2 < n_kept; k += 3) {
        const adsb_aircraft_modes &a = kept[k], &b = kept[(k * 7 + 1) % n_kept], &c = kept[(k * 13 + 2) % n_kept];
        CHECK(same_bytes(merge(merge(a, b), c), merge(a, merge(b, c))));
    }

    // saturation: counts preloaded with 2^32 - 2 and 2^32 - 1
    for (uint32_t start : {0xFFFFFFFEu, 0xFFFFFFFFu}) {
        adsb_aircraft_modes big = empty;
        big.n_replies = big.n_allcall = big.n_surveillance = big.n_airair = start;
        for (unsigned df : {0u, 4u, 5u, 11u, 16u, 20u, 21u, 24u, 17u}) {
            std::memset(&rec, 0, sizeof(rec));
            rec.df = (uint8_t)df;
            rec.kind = ADSB_MODES_KNOWN;
            adsb_aircraft_modes a = big;
            for (int step = 0; step < 3; ++step) a = merge(a, one(rec, 1.0));
            const bool reply = df != 17;
            CHECK(a.n_replies == (reply ? 0xFFFFFFFFu : start));
            CHECK(a.n_allcall == (df == 11 ? 0xFFFFFFFFu : start));
            CHECK(a.n_surveillance == ((df == 4 || df == 5 || df == 20 || df == 21) ? 0xFFFFFFFFu : start));
            CHECK(a.n_airair == ((df == 0 || df == 16) ? 0xFFFFFFFFu : start));
        }
        // a saturated part still is a source of GROUND
        adsb_aircraft_modes part = big;
        part.flags = ADSB_TRACK_MODES_GROUND;
        adsb_aircraft_modes into = empty;
        CHECK((merge(into, part).flags & ADSB_TRACK_MODES_GROUND) != 0);
    }

    // later wins at equal times
    {
        adsb_modes_rec x, y;
        std::memset(&x, 0, sizeof(x));
        std::memset(&y, 0, sizeof(y));
        x.kind = y.kind = ADSB_MODES_KNOWN;
        x.df = 20; x.flags = ADSB_MODES_ALT | ADSB_MODES_CALLSIGN | ADSB_MODES_GROUND | ADSB_MODES_ALERT; x.altitude_ft = 1000; x.fs = 3;
        std::memcpy(x.callsign, "FIRST___", 8);
        y.df = 21; y.flags = ADSB_MODES_SQUAWK | ADSB_MODES_CALLSIGN | ADSB_MODES_SPI; y.squawk = 7700; y.fs = 5;
        std::memcpy(y.callsign, "SECOND__", 8);
        const adsb_aircraft_modes xy = merge(one(x, 2.0), one(y, 2.0)), yx = merge(one(y, 2.0), one(x, 2.0));
        CHECK(std::memcmp(xy.callsign, "SECOND__", 8) == 0 && xy.fs == 5 && xy.last_df == 21 && !(xy.flags & ADSB_TRACK_MODES_GROUND));
        CHECK((xy.flags & ADSB_TRACK_MODES_SPI) && !(xy.flags & ADSB_TRACK_MODES_ALERT) && xy.altitude_ft == 1000 && xy.squawk == 7700);
        CHECK(std::memcmp(yx.callsign, "FIRST___", 8) == 0 && yx.fs == 3 && yx.last_df == 20 && (yx.flags & ADSB_TRACK_MODES_GROUND));
        CHECK((yx.flags & ADSB_TRACK_MODES_ALERT) && !(yx.flags & ADSB_TRACK_MODES_SPI) && xy.n_surveillance == 2 && yx.n_replies == 2);
    }
    std::printf("track_modes_edges: %lu calls (%lu accepted), %lu merges, %d failures\n", n_calls, n_accepted, n_merges, fails);
    return fails ? 1 : 0;
}
