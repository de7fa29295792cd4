// track_es_edges.cpp -- stand-alone sanitizer run of the CPU mirror of the track table's extended squitter step
// (adsb_host_es_resolve, adsb_host_track_es_of and adsb_host_track_es_merge, air_rs_amd/csrc/host/adsb_track_es.cpp,
// which compiles the text the device compiles: air_rs_amd/csrc/adsb_track_es.h).  Exact-size heap buffers for every
// record in and out, so that a read or write beside them is a heap-buffer-overflow; every state byte with every type
// code and present bit pattern that matters, versions 0..7 and unknown, supplements of every value, NaN, infinite,
// negative and denormal times, ages at the limit, one ulp over it and negative, limits of 0 and +inf, counts at
// 2^32 - 2 and 2^32 - 1, and folds in both groupings.  Host sources only, no device:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/host/track_es_edges.cpp
//       air_rs_amd/csrc/host/adsb_track_es.cpp air_rs_amd/csrc/host/adsb_es.cpp -o /tmp/track_es_edges
//       && /tmp/track_es_edges                                                           (one command)
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

static unsigned long n_resolves = 0, n_positions = 0, n_stale = 0, n_ones = 0, n_merges = 0;

template <class T>
static T *heap_copy(const T &x)
{
    T *p = static_cast<T *>(std::malloc(sizeof(T)));
    std::memcpy(p, &x, sizeof(T));
    return p;
}

static bool same_bytes(const adsb_aircraft_es &a, const adsb_aircraft_es &b) { return std::memcmp(&a, &b, sizeof(a)) == 0; }

// the per-frame output on exact-size heap copies, and the invariants that hold whatever the inputs
static adsb_frame_integrity resolve(const adsb_es_rec &rec, double t, const adsb_aircraft_es *held, const adsb_es_track_cfg *cfg)
{
    adsb_es_rec *r = heap_copy(rec);
    adsb_aircraft_es *h = held ? heap_copy(*held) : nullptr;
    adsb_es_track_cfg *c = cfg ? heap_copy(*cfg) : nullptr;
    adsb_frame_integrity *out = static_cast<adsb_frame_integrity *>(std::malloc(sizeof(adsb_frame_integrity)));
    std::memset(out, 0xEE, sizeof(*out));
    CHECK(adsb_host_es_resolve(r, t, h, c, out) == ADSB_OK);
    const adsb_frame_integrity o = *out;
    ++n_resolves;
    const bool counted = rec.state != ADSB_ES_NOT_ES && rec.state != ADSB_ES_FOREIGN;
    CHECK(((o.flags & ADSB_TRACK_ES_COUNTED) != 0) == counted);
    if (!counted) CHECK(o.rc_dm == 0 && o.nic == 0 && o.version == 0 && o.supp == 0 && o.flags == 0);
    if (counted && rec.state != ADSB_ES_POSITION) CHECK(o.flags == ADSB_TRACK_ES_COUNTED && o.rc_dm == 0 && o.nic == 0 && o.supp == 0);
    if (counted) CHECK(o.version == (held && held->version_time == held->version_time ? held->version : ADSB_ES_VERSION_UNKNOWN));
    if (o.flags & ADSB_TRACK_ES_POSITION) {
        ++n_positions;
        uint32_t nic = 99, rc = 99;
        CHECK(adsb_host_es_integrity(rec.type_code, o.version, o.supp, &nic, &rc) == ADSB_OK); // the table is called, not restated
        CHECK(nic == o.nic && rc == o.rc_dm && o.supp < 8);
        CHECK(((o.flags & ADSB_TRACK_ES_VERSIONED) != 0) == (held && held->version_time == held->version_time));
        if (o.flags & (ADSB_TRACK_ES_STALE_A | ADSB_TRACK_ES_STALE_C)) ++n_stale;
        if (o.flags & ADSB_TRACK_ES_STALE_A) CHECK(!(o.supp & 1u));
        if (o.flags & ADSB_TRACK_ES_STALE_C) CHECK(!(o.supp & 4u));
    }
    std::free(r), std::free(h), std::free(c), std::free(out);
    return o;
}

static adsb_aircraft_es one(const adsb_es_rec &rec, const adsb_frame_integrity &f, double t)
{
    adsb_es_rec *r = heap_copy(rec);
    adsb_frame_integrity *fi = heap_copy(f);
    adsb_aircraft_es *out = static_cast<adsb_aircraft_es *>(std::malloc(sizeof(adsb_aircraft_es)));
    std::memset(out, 0xEE, sizeof(*out));
    CHECK(adsb_host_track_es_of(r, fi, t, out) == ADSB_OK);
    const adsb_aircraft_es a = *out;
    ++n_ones;
    CHECK(a.n_es == ((f.flags & ADSB_TRACK_ES_COUNTED) ? 1u : 0u) && a.reserved == 0);
    std::free(r), std::free(fi), std::free(out);
    return a;
}

static adsb_aircraft_es merge(const adsb_aircraft_es &into, const adsb_aircraft_es &later)
{
    adsb_aircraft_es *a = heap_copy(into), *b = heap_copy(later);
    CHECK(adsb_host_track_es_merge(a, b) == ADSB_OK);
    CHECK(same_bytes(*b, later)); // later is only read
    const adsb_aircraft_es o = *a;
    ++n_merges;
    std::free(a), std::free(b);
    return o;
}

int main()
{
    const double inf = std::numeric_limits<double>::infinity(), nan = std::nan(""), denorm = std::numeric_limits<double>::denorm_min();
    const adsb_es_rec none{};
    const adsb_frame_integrity nothing{};
    const adsb_aircraft_es empty = one(none, nothing, 0.0);
    for (int k = 0; k < 5; ++k) CHECK(std::isnan(empty.time[k]));
    CHECK(std::isnan(empty.version_time) && std::isnan(empty.nic_a_time) && std::isnan(empty.nic_c_time) && std::isnan(empty.position_time));
    CHECK(empty.n_es == 0 && empty.n_position == 0 && empty.has == 0 && empty.category == 0 && empty.rc_dm == 0);
    CHECK(same_bytes(merge(empty, empty), empty));

    // every state x type code x the present bits the rule reads, against held records of every version and supplement
    const double times[] = {0.0, 1.0, 59.0, 60.0, std::nextafter(60.0, 100.0), 61.0, -1.0, 1e300, denorm, inf, -inf, nan};
    const adsb_es_track_cfg limits[] = {{60.0, {0, 0}}, {0.0, {0, 0}}, {inf, {0, 0}}, {denorm, {0, 0}}};
    adsb_aircraft_es folded = empty, left = empty, right = empty;
    unsigned long k = 0;
    for (unsigned state = 0; state < 12; ++state)
        for (unsigned tc = 0; tc < 32; ++tc)
            for (unsigned bits = 0; bits < 8; ++bits) {
                adsb_es_rec rec{};
                rec.state = (uint8_t)state;
                rec.type_code = (uint8_t)tc;
                rec.subtype = (uint8_t)(bits & 1u) + (bits == 7 ? 6 : 0);
                rec.version = (uint8_t)((tc + bits) & 7u);
                rec.present = ((bits & 1u) ? ADSB_ES_HAS_VERSION | ADSB_ES_HAS_NIC_A : 0u) | ((bits & 2u) ? ADSB_ES_HAS_NIC_B | ADSB_ES_HAS_NAC_V : 0u) |
                              ((bits & 4u) ? ADSB_ES_HAS_NIC_C | ADSB_ES_HAS_CATEGORY : 0u);
                rec.nic_a = (uint8_t)(tc & 1u), rec.nic_b = (uint8_t)(tc >> 1 & 1u) | (bits == 7 ? 0xFE : 0), rec.nic_c = (uint8_t)(tc >> 2 & 1u);
                rec.nac_v = 5, rec.category = 0xA3, rec.flags = 0x7FF, rec.value = 0xFFFFFFFFu, rec.half[0] = rec.half[1] = 0xFFFF;
                for (unsigned held_kind = 0; held_kind < 6; ++held_kind) {
                    adsb_aircraft_es held = empty;
                    if (held_kind >= 1) held.version = (uint8_t)(held_kind == 5 ? 0xFF : held_kind - 1), held.version_time = 0.5;
                    if (held_kind >= 2) held.nic_a = 1, held.nic_a_time = times[(k + 1) % 12];
                    if (held_kind >= 3) held.nic_c = 0xFF, held.nic_c_time = times[(k + 5) % 12];
                    const double t = times[k % 12];
                    const adsb_frame_integrity f = resolve(rec, t, held_kind ? &held : nullptr, (k & 3) ? &limits[k & 3] : nullptr);
                    const adsb_aircraft_es part = one(rec, f, t);
                    // into followed by the part, in both groupings
                    folded = merge(folded, part);
                    if (k & 1) right = merge(right, part);
                    else if (right.n_es) left = merge(left, right), right = part;
                    else left = merge(left, part);
                    // the identity, for every time the store can give a frame (with a NaN time, which it cannot, a part
                    // says of itself that it holds no block)
                    if (t == t) CHECK(same_bytes(merge(empty, part), part) && same_bytes(merge(part, empty), part));
                    ++k;
                }
            }
    CHECK(same_bytes(merge(left, right), folded));
    CHECK(folded.n_es > 1000 && folded.n_position > 100 && folded.has != 0 && folded.category == 0xA3);

    // the age limit: exactly max_age_s old is usable, one ulp older is stale, a negative age is stale, NaN is stale
    adsb_es_rec pos{};
    pos.state = ADSB_ES_POSITION, pos.type_code = 11, pos.present = ADSB_ES_HAS_NIC_B, pos.nic_b = 1;
    adsb_aircraft_es held = empty;
    held.version = 2, held.version_time = 0.0, held.nic_a = 1, held.nic_a_time = 0.0;
    const adsb_es_track_cfg cfg60{60.0, {0, 0}}, cfg_inf{inf, {0, 0}};
    adsb_frame_integrity f = resolve(pos, 60.0, &held, &cfg60);
    CHECK(f.nic == 9 && f.rc_dm == 750 && f.supp == 3 && f.flags == (ADSB_TRACK_ES_COUNTED | ADSB_TRACK_ES_POSITION | ADSB_TRACK_ES_VERSIONED));
    f = resolve(pos, std::nextafter(60.0, 100.0), &held, &cfg60);
    CHECK(f.nic == 8 && f.rc_dm == 1852 && f.supp == 2 && (f.flags & ADSB_TRACK_ES_STALE_A));
    f = resolve(pos, 1e300, &held, &cfg_inf);
    CHECK(f.nic == 9 && !(f.flags & ADSB_TRACK_ES_STALE_A));
    held.nic_a_time = 61.0;
    f = resolve(pos, 60.0, &held, &cfg_inf);
    CHECK(f.nic == 8 && (f.flags & ADSB_TRACK_ES_STALE_A));
    f = resolve(pos, nan, &held, &cfg_inf);
    CHECK(f.nic == 8 && (f.flags & ADSB_TRACK_ES_STALE_A));
    f = resolve(pos, 5.0, nullptr, nullptr);
    CHECK(f.nic == 0 && f.rc_dm == 1852 && f.version == ADSB_ES_VERSION_UNKNOWN && f.flags == (ADSB_TRACK_ES_COUNTED | ADSB_TRACK_ES_POSITION));

    // counts saturate
    const adsb_aircraft_es p1 = one(pos, f, 5.0);
    CHECK(p1.n_es == 1 && p1.n_position == 1 && p1.rc_dm == 1852 && p1.position_tc == 11 && p1.nic_b == 1 && p1.position_time == 5.0);
    for (uint32_t start : {0xFFFFFFFDu, 0xFFFFFFFEu, 0xFFFFFFFFu}) {
        adsb_aircraft_es big = p1;
        big.n_es = big.n_position = start;
        const adsb_aircraft_es got = merge(big, p1);
        const uint32_t want = start == 0xFFFFFFFFu ? start : start + 1u;
        CHECK(got.n_es == want && got.n_position == want);
    }

    // arguments
    adsb_frame_integrity out{};
    adsb_aircraft_es a = empty;
    CHECK(adsb_host_es_resolve(nullptr, 0.0, nullptr, nullptr, &out) == ADSB_E_ARG);
    CHECK(adsb_host_es_resolve(&pos, 0.0, nullptr, nullptr, nullptr) == ADSB_E_ARG);
    for (double bad : {nan, -1.0, -inf}) {
        const adsb_es_track_cfg c{bad, {0, 0}};
        CHECK(adsb_host_es_resolve(&pos, 0.0, nullptr, &c, &out) == ADSB_E_ARG);
    }
    CHECK(adsb_host_track_es_of(nullptr, &out, 0.0, &a) == ADSB_E_ARG && adsb_host_track_es_of(&pos, nullptr, 0.0, &a) == ADSB_E_ARG &&
          adsb_host_track_es_of(&pos, &out, 0.0, nullptr) == ADSB_E_ARG);
    CHECK(adsb_host_track_es_merge(nullptr, &a) == ADSB_E_ARG && adsb_host_track_es_merge(&a, nullptr) == ADSB_E_ARG);

    std::printf("%lu resolves (%lu positions, %lu with a stale supplement), %lu single-frame records, %lu merges: %s\n", n_resolves,
                n_positions, n_stale, n_ones, n_merges, fails ? "FAILED" : "clean");
    return fails ? 1 : 0;
}
