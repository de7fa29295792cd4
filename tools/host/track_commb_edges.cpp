// track_commb_edges.cpp -- stand-alone sanitizer run of the CPU mirror of the track table's Comm-B step
// (adsb_host_commb_settle, adsb_host_commb_reference, adsb_host_track_commb_of and adsb_host_track_commb_merge,
// air_rs_amd/csrc/host/adsb_track_commb.cpp, which compiles the text the device compiles:
// air_rs_amd/csrc/adsb_track_commb.h).  Exact-size heap buffers for every record in and out, so that a read or write
// beside them is a heap-buffer-overflow; every state and bds byte, payloads that read as 5,0 and as 6,0 against
// references of every subtype with extreme components, rates, headings and airspeeds, limits of 0 and 2^32 - 1, NaN,
// infinite and denormal times and ages, counts at 2^32 - 2 and 2^32 - 1, and folds in both groupings.  Host sources
// only, no device:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/host/track_commb_edges.cpp
//       air_rs_amd/csrc/host/adsb_track_commb.cpp air_rs_amd/csrc/host/adsb_commb.cpp -o /tmp/track_commb_edges
//       && /tmp/track_commb_edges                                                        (one command)
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

static unsigned long n_settles = 0, n_settled = 0, n_ones = 0, n_merges = 0;

template <class T>
static T *heap_copy(const T &x)
{
    T *p = static_cast<T *>(std::malloc(sizeof(T)));
    std::memcpy(p, &x, sizeof(T));
    return p;
}

static bool same_bytes(const adsb_aircraft_commb &a, const adsb_aircraft_commb &b) { return std::memcmp(&a, &b, sizeof(a)) == 0; }

// MB from {first bit (1-based), width, value} triples into frame bytes 4..10 of a DF20 frame
static void put(uint8_t bytes[14], unsigned a, unsigned n, uint32_t v)
{
    for (unsigned k = 0; k < n; ++k) {
        const unsigned bit = a - 1 + k; // 0-based MB bit
        const uint8_t mask = (uint8_t)(0x80u >> (bit & 7));
        if (v >> (n - 1 - k) & 1u) bytes[4 + (bit >> 3)] |= mask;
        else bytes[4 + (bit >> 3)] &= (uint8_t)~mask;
    }
}

// the per-frame output on exact-size heap copies, and the invariants that hold whatever the inputs
static adsb_commb_rec settle(const uint8_t bytes[14], const adsb_commb_rec &rec, const adsb_velocity *ref, double t,
                             const adsb_commb_settle_cfg *cfg)
{
    uint8_t *b = static_cast<uint8_t *>(std::malloc(14));
    std::memcpy(b, bytes, 14);
    adsb_commb_rec *r = heap_copy(rec), *out = static_cast<adsb_commb_rec *>(std::malloc(sizeof(adsb_commb_rec)));
    adsb_velocity *v = ref ? heap_copy(*ref) : nullptr;
    adsb_commb_settle_cfg *c = cfg ? heap_copy(*cfg) : nullptr;
    std::memset(out, 0xEE, sizeof(*out));
    CHECK(adsb_host_commb_settle(b, r, v, t, c, out) == ADSB_OK);
    CHECK(std::memcmp(r, &rec, sizeof(rec)) == 0); // read only
    const adsb_commb_rec o = *out;
    CHECK(adsb_host_commb_settle(b, r, v, t, c, r) == ADSB_OK && std::memcmp(r, &o, sizeof(o)) == 0); // in place
    std::free(c);
    std::free(v);
    std::free(out);
    std::free(r);
    std::free(b);
    ++n_settles;
    if (o.state == ADSB_COMMB_SETTLED && rec.state != ADSB_COMMB_SETTLED) {
        ++n_settled;
        CHECK(rec.state == ADSB_COMMB_AMBIGUOUS && rec.candidates == (ADSB_COMMB_C50 | ADSB_COMMB_C60) && ref);
        CHECK((o.bds == 0x50 || o.bds == 0x60) && o.candidates == rec.candidates && o.n_candidates == rec.n_candidates);
        CHECK(o.reserved == rec.reserved && o.word == 0 && (o.status & ~0x1Fu) == 0);
        adsb_commb_rec as;
        std::memset(&as, 0, sizeof(as));
        CHECK(adsb_host_commb_as(bytes, o.bds, &as) == ADSB_OK);
        CHECK(as.status == o.status && std::memcmp(as.value, o.value, sizeof(o.value)) == 0);
    } else {
        CHECK(std::memcmp(&o, &rec, sizeof(o)) == 0);
    }
    return o;
}

static adsb_aircraft_commb one(const adsb_commb_rec &rec, double time)
{
    adsb_commb_rec *r = heap_copy(rec);
    adsb_aircraft_commb *out = static_cast<adsb_aircraft_commb *>(std::malloc(sizeof(adsb_aircraft_commb)));
    std::memset(out, 0xEE, sizeof(*out));
    CHECK(adsb_host_track_commb_of(r, time, out) == ADSB_OK);
    const adsb_aircraft_commb a = *out;
    std::free(out);
    std::free(r);
    ++n_ones;
    CHECK(a.n_commb == (rec.state != ADSB_COMMB_NOT_COMMB ? 1u : 0u));
    CHECK(a.n_settled == (rec.state == ADSB_COMMB_SETTLED ? 1u : 0u) && a.n_none == (rec.state == ADSB_COMMB_NONE ? 1u : 0u));
    CHECK(a.n_ambiguous == (rec.state == ADSB_COMMB_AMBIGUOUS ? 1u : 0u));
    const bool valued = rec.state == ADSB_COMMB_ONE || rec.state == ADSB_COMMB_SETTLED;
    for (const adsb_commb_block *k : {&a.bds40, &a.bds50, &a.bds60}) {
        const unsigned bds = k == &a.bds40 ? 0x40u : k == &a.bds50 ? 0x50u : 0x60u;
        if (valued && rec.bds == bds) {
            CHECK(std::memcmp(&k->time, &time, 8) == 0 && std::memcmp(k->value, rec.value, sizeof(rec.value)) == 0);
            CHECK(k->status == rec.status && k->settled == (rec.state == ADSB_COMMB_SETTLED ? 1u : 0u));
        } else {
            CHECK(std::isnan(k->time) && k->status == 0 && k->settled == 0 && k->value[0] == 0 && k->value[4] == 0);
        }
    }
    CHECK(a.capability == ((rec.state == ADSB_COMMB_ONE && rec.bds == 0x17) ? rec.word : 0u));
    if (rec.state == ADSB_COMMB_ONE && rec.bds == 0x30) CHECK(a.ra_word == rec.word && std::memcmp(&a.ra_time, &time, 8) == 0);
    else CHECK(a.ra_word == 0 && std::isnan(a.ra_time));
    return a;
}

static adsb_aircraft_commb merge(const adsb_aircraft_commb &into, const adsb_aircraft_commb &later)
{
    adsb_aircraft_commb *a = heap_copy(into), *b = heap_copy(later);
    CHECK(adsb_host_track_commb_merge(a, b) == ADSB_OK);
    CHECK(same_bytes(*b, later)); // the later record is read only
    const adsb_aircraft_commb o = *a;
    std::free(b);
    std::free(a);
    ++n_merges;
    return o;
}

static adsb_velocity reference(const uint8_t bytes[14], double time)
{
    uint8_t *b = static_cast<uint8_t *>(std::malloc(14));
    std::memcpy(b, bytes, 14);
    adsb_velocity *v = static_cast<adsb_velocity *>(std::malloc(sizeof(adsb_velocity)));
    std::memset(v, 0xEE, sizeof(*v));
    CHECK(adsb_host_commb_reference(b, time, v) == ADSB_OK);
    const adsb_velocity o = *v;
    std::free(v);
    std::free(b);
    CHECK(o.subtype <= 4 && o.reserved == 0 && (o.flags & ~7u) == 0);
    if (o.subtype == 0) CHECK(std::isnan(o.time) && o.flags == 0);
    return o;
}

int main()
{
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    const double times[] = {0.0, -0.0, 1.5, 10.0, 1e300, -1e300, 5e-324, inf, -inf, nan};
    adsb_commb_rec rec;
    std::memset(&rec, 0, sizeof(rec));
    const adsb_aircraft_commb empty = one(rec, 3.0);
    CHECK(std::isnan(empty.bds40.time) && std::isnan(empty.bds50.time) && std::isnan(empty.bds60.time) && std::isnan(empty.ra_time));
    uint8_t frame[14] = {20 << 3, 0, 2, 0x9c};
    adsb_velocity vel;
    CHECK(adsb_host_commb_settle(nullptr, &rec, nullptr, 0.0, nullptr, &rec) == ADSB_E_ARG);
    CHECK(adsb_host_commb_settle(frame, nullptr, nullptr, 0.0, nullptr, &rec) == ADSB_E_ARG);
    CHECK(adsb_host_commb_settle(frame, &rec, nullptr, 0.0, nullptr, nullptr) == ADSB_E_ARG);
    for (double bad : {nan, -1.0, -inf}) {
        const adsb_commb_settle_cfg cfg = {bad, 40, 1000};
        CHECK(adsb_host_commb_settle(frame, &rec, nullptr, 0.0, &cfg, &rec) == ADSB_E_ARG);
    }
    CHECK(adsb_host_commb_reference(nullptr, 0.0, &vel) == ADSB_E_ARG && adsb_host_commb_reference(frame, 0.0, nullptr) == ADSB_E_ARG);
    adsb_aircraft_commb scratch = empty;
    CHECK(adsb_host_track_commb_of(nullptr, 0.0, &scratch) == ADSB_E_ARG && adsb_host_track_commb_of(&rec, 0.0, nullptr) == ADSB_E_ARG);
    CHECK(adsb_host_track_commb_merge(nullptr, &scratch) == ADSB_E_ARG && adsb_host_track_commb_merge(&scratch, nullptr) == ADSB_E_ARG);

    // references: every subtype 0-7, components, headings, airspeeds and rates at 0, 1 and their maxima, both signs
    static adsb_velocity refs[4096];
    unsigned n_refs = 0;
    for (unsigned st = 0; st < 8; ++st)
        for (uint32_t f14 : {0u, 1u, 2u, 431u, 1023u})
            for (uint32_t f25 : {0u, 1u, 2u, 361u, 1023u})
                for (uint32_t vr : {0u, 1u, 11u, 511u})
                    for (unsigned signs = 0; signs < 8; ++signs) {
                        uint8_t v[14] = {0x8D, 0x4B, 0x12, 0x34};
                        put(v, 1, 5, 19);
                        put(v, 6, 3, st);
                        put(v, 14, 1, signs & 1);
                        put(v, 15, 10, f14);
                        put(v, 25, 1, signs >> 1 & 1);
                        put(v, 26, 10, f25);
                        put(v, 36, 1, 1);
                        put(v, 37, 1, signs >> 2 & 1);
                        put(v, 38, 9, vr);
                        const adsb_velocity r = reference(v, times[(st + f14 + vr + signs) % 10]);
                        CHECK((r.subtype != 0) == (st >= 1 && st <= 4));
                        if (r.subtype && n_refs < 4096) refs[n_refs++] = r;
                    }
    CHECK(n_refs > 1000);

    // payloads that read as 5,0 and as 6,0 (status bits 1, 12/13, 24, 35, 46 in their combinations), every one against
    // every reference, at several frame times and limits
    const adsb_commb_settle_cfg cfgs[] = {{10.0, 40, 1000}, {0.0, 0, 0}, {inf, 0xFFFFFFFFu, 0xFFFFFFFFu}, {1e-300, 1, 1}, {10.0, 0xFFFFFFFFu, 0}};
    static adsb_aircraft_commb kept[4096];
    unsigned n_kept = 0, n_both = 0;
    for (unsigned pattern = 0; pattern < 64; ++pattern) {
        uint8_t b[14] = {20 << 3, 0, 2, 0x9c};
        if (pattern & 1) { put(b, 1, 1, 1); put(b, 2, 10, (pattern & 32) ? 0x3DFu : 0x21Fu); }    // roll / heading
        if (pattern & 2) { put(b, 12, 1, 1); put(b, 13, 11, 0x400u | (pattern * 7u)); }             // track / IAS
        if (pattern & 4) { put(b, 24, 1, 1); put(b, 25, 10, 215); }                                  // ground speed / Mach
        if (pattern & 8) { put(b, 35, 1, 1); put(b, 36, 10, (pattern & 32) ? 0x3ECu : 20u); }       // track rate / baro rate
        if (pattern & 16) { put(b, 46, 1, 1); put(b, 47, 10, 180); }                                 // TAS / inertial rate
        adsb_commb_rec first;
        std::memset(&first, 0, sizeof(first));
        CHECK(adsb_host_commb((const adsb_frame *)nullptr, 0, nullptr, nullptr) == ADSB_OK);
        adsb_frame fr;
        std::memset(&fr, 0, sizeof(fr));
        std::memcpy(fr.bytes, b, 14);
        CHECK(adsb_host_commb(&fr, 1, &first, nullptr) == ADSB_OK);
        const bool both = first.state == ADSB_COMMB_AMBIGUOUS && first.candidates == (ADSB_COMMB_C50 | ADSB_COMMB_C60);
        n_both += both ? 1u : 0u;
        for (unsigned r = 0; r < n_refs; r += both ? 1 : 37)
            for (unsigned c = 0; c < 5; ++c) {
                const double t = times[(r + c + pattern) % 10];
                const adsb_commb_rec o = settle(b, first, &refs[r], t, &cfgs[c]);
                if (!both) CHECK(o.state != ADSB_COMMB_SETTLED);
                if (n_kept < 4096 && (r * 5 + c) % 97 == 0 && !std::isnan(t)) kept[n_kept++] = one(o, t);
            }
        settle(b, first, nullptr, 1.0, nullptr); // no reference, default limits
    }
    CHECK(n_both >= 8 && n_settled > 1000 && n_kept > 500);

    // every state and bds byte, status and values at their extremes
    for (unsigned state = 0; state < 256; ++state)
        for (unsigned bds : {0u, 0x10u, 0x17u, 0x20u, 0x30u, 0x40u, 0x50u, 0x60u, 0x44u, 0xFFu}) {
            std::memset(&rec, 0xA5, sizeof(rec));
            rec.state = (uint8_t)state;
            rec.bds = (uint8_t)bds;
            rec.status = (uint16_t)(state * 257u);
            rec.value[0] = std::numeric_limits<int32_t>::min();
            rec.value[4] = std::numeric_limits<int32_t>::max();
            rec.word = (state & 1) ? 0u : 0xFFFFFFFFu;
            if (state == ADSB_COMMB_ONE && bds == 0x17 && rec.word == 0) continue; // writes nothing: checked below
            const double t = times[(state + bds) % 10];
            const adsb_aircraft_commb a = one(rec, t);
            if (n_kept < 4096 && state < 8 && !std::isnan(t)) kept[n_kept++] = a;
            settle(frame, rec, &refs[state % n_refs], 1.0, nullptr);
        }
    std::memset(&rec, 0, sizeof(rec));
    rec.state = ADSB_COMMB_ONE;
    rec.bds = 0x17;
    {
        adsb_aircraft_commb a;
        CHECK(adsb_host_track_commb_of(&rec, 1.0, &a) == ADSB_OK && a.capability == 0 && a.n_commb == 1);
    }

    // the empty record is the identity (of parts whose frame time is no NaN: a block with a NaN time is none, and the
    // store's frame times are finite); folds in both groupings agree
    for (unsigned k = 0; k < n_kept; ++k) {
        CHECK(same_bytes(merge(empty, kept[k]), kept[k]));
        CHECK(same_bytes(merge(kept[k], empty), kept[k]));
    }
    for (unsigned k = 0; k + 2 < n_kept; k += 3) {
        const adsb_aircraft_commb &a = kept[k], &b = kept[(k * 7 + 1) % n_kept], &c = kept[(k * 13 + 2) % n_kept];
        CHECK(same_bytes(merge(merge(a, b), c), merge(a, merge(b, c))));
    }

    // saturation: counts preloaded with 2^32 - 2 and 2^32 - 1
    for (uint32_t start : {0xFFFFFFFEu, 0xFFFFFFFFu}) {
        adsb_aircraft_commb big = empty;
        big.n_commb = big.n_settled = big.n_ambiguous = big.n_none = start;
        for (unsigned state : {1u, 2u, 3u, 4u, 5u}) {
            std::memset(&rec, 0, sizeof(rec));
            rec.state = (uint8_t)state;
            rec.bds = 0x50;
            adsb_aircraft_commb a = big;
            for (int step = 0; step < 3; ++step) a = merge(a, one(rec, 1.0));
            CHECK(a.n_commb == 0xFFFFFFFFu);
            CHECK(a.n_none == (state == ADSB_COMMB_NONE ? 0xFFFFFFFFu : start));
            CHECK(a.n_ambiguous == (state == ADSB_COMMB_AMBIGUOUS ? 0xFFFFFFFFu : start));
            CHECK(a.n_settled == (state == ADSB_COMMB_SETTLED ? 0xFFFFFFFFu : start));
        }
    }

    // later wins at equal times
    {
        adsb_commb_rec x, y;
        std::memset(&x, 0, sizeof(x));
        std::memset(&y, 0, sizeof(y));
        x.state = ADSB_COMMB_ONE; x.bds = 0x50; x.status = 4; x.value[2] = 430;
        y.state = ADSB_COMMB_SETTLED; y.bds = 0x50; y.status = 4; y.value[2] = 250;
        const adsb_aircraft_commb xy = merge(one(x, 2.0), one(y, 2.0)), yx = merge(one(y, 2.0), one(x, 2.0));
        CHECK(xy.bds50.value[2] == 250 && xy.bds50.settled == 1 && yx.bds50.value[2] == 430 && yx.bds50.settled == 0);
        CHECK(xy.n_commb == 2 && xy.n_settled == 1 && yx.n_settled == 1);
    }
    std::printf("track_commb_edges: %lu settles (%lu settled), %lu contributions, %lu merges, %d failures\n", n_settles,
                n_settled, n_ones, n_merges, fails);
    return fails ? 1 : 0;
}
