// es_edges.cpp -- stand-alone sanitizer run of the CPU mirror of the extended squitter status stage (adsb_host_es and
// adsb_host_es_integrity, air_rs_amd/csrc/host/adsb_es.cpp, which compiles the text the device compiles:
// air_rs_amd/csrc/adsb_es.h).  Exact-size heap buffers for the frames in and the records out, so that a read or write
// beside them is a heap-buffer-overflow; every DF with every low three bits of byte 0, every type code with every
// subtype over an empty and a full payload and over every single bit and every pair of bits of the payload, every
// squawk, and a few hundred thousand random frames.  What holds whatever the input is checked on every record; the
// integrity function takes every type code, version and supplement set and values far outside them.  Host sources
// only, no device:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/host/es_edges.cpp
//       air_rs_amd/csrc/host/adsb_es.cpp -o /tmp/es_edges && /tmp/es_edges   (one command)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <vector>

#include "../../include/adsb_host.h"

static int fails = 0;
#define CHECK(x)                                                     \
    do {                                                             \
        if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); ++fails; } \
    } while (0)

static unsigned long n_frames = 0, n_state[ADSB_ES_STATES] = {};

// a frame of format df around ME = the 56-bit number me
static adsb_frame frame_of(uint64_t me, unsigned df = 17, unsigned low3 = 5)
{
    adsb_frame f;
    std::memset(&f, 0xA5, sizeof(f));
    f.bytes[0] = (uint8_t)(df << 3 | low3);
    for (int k = 0; k < 7; ++k) f.bytes[4 + k] = (uint8_t)(me >> (48 - 8 * k));
    return f;
}

// bit a (1..56) of ME as a mask of the 56-bit number
static uint64_t bit(unsigned a) { return 1ull << (56 - a); }
// the n bits from bit a set to x
static uint64_t field(unsigned a, unsigned n, uint64_t x) { return (x & ((1ull << n) - 1)) << (57 - a - n); }
static uint64_t tc_st(unsigned tc, unsigned st) { return field(1, 5, tc) | field(6, 3, st); }

static bool rc_of_the_table(uint32_t rc)
{
    for (uint32_t x : {75u, 250u, 750u, 1852u, 3704u, 5556u, 9260u, 11112u, 18520u, 37040u, 74080u, 148160u, 185200u, 370400u})
        if (rc == x) return true;
    return false;
}

// the invariants of one record, whatever the frame
static void check_record(const adsb_frame &f, const adsb_es_rec &r)
{
    const unsigned df = f.bytes[0] >> 3, low3 = f.bytes[0] & 7, tc = f.bytes[4] >> 3, st = f.bytes[4] & 7;
    CHECK(r.state < ADSB_ES_STATES && r.reserved == 0 && r.present < (1u << 27) && r.flags < (1u << 11));
    n_state[r.state < ADSB_ES_STATES ? r.state : 0] += 1;
    if (df != 17 && df != 18) CHECK(r.state == ADSB_ES_NOT_ES);
    else if (df == 18 && low3 > 1) CHECK(r.state == ADSB_ES_FOREIGN);
    else CHECK(r.state >= ADSB_ES_CATEGORY && r.type_code == tc);
    if (r.state <= ADSB_ES_FOREIGN) {
        adsb_es_rec zero;
        std::memset(&zero, 0, sizeof(zero));
        zero.state = r.state;
        CHECK(std::memcmp(&zero, &r, sizeof(r)) == 0);
        return;
    }
    CHECK(r.subtype == (r.state == ADSB_ES_CATEGORY || r.state == ADSB_ES_POSITION ? 0u : tc == 29 ? st >> 1 : st));
    CHECK(r.nic_a <= 1 && r.nic_b <= 1 && r.nic_c <= 1 && r.nac_p <= 15 && r.nac_v <= 7 && r.sil <= 3 && r.sil_supplement <= 1 &&
          r.gva <= 3 && r.sda <= 3 && r.nic_baro <= 1 && r.emergency <= 7 && r.length_width <= 15 && r.version <= 7);
    switch (r.state) {
    case ADSB_ES_CATEGORY:
        CHECK(r.present == ADSB_ES_HAS_CATEGORY && (r.category >> 4) == 0xE - tc && (r.category & 15u) == st && r.flags == 0);
        break;
    case ADSB_ES_POSITION:
        CHECK((r.present & ~(ADSB_ES_HAS_NIC_B | ADSB_ES_HAS_RC)) == 0 && r.flags == 0 && r.half[0] == 0 && r.half[1] == 0);
        CHECK(((r.present & ADSB_ES_HAS_NIC_B) != 0) == (tc >= 9 && tc <= 18));
        CHECK(r.present & ADSB_ES_HAS_RC ? rc_of_the_table(r.value) : r.value == 0);
        break;
    case ADSB_ES_VELOCITY:
        CHECK(r.present == (ADSB_ES_HAS_NAC_V | ADSB_ES_HAS_VELOCITY_FLAGS) && (r.flags & ~(ADSB_ES_INTENT_CHANGE | ADSB_ES_IFR)) == 0);
        break;
    case ADSB_ES_EMERGENCY:
        CHECK(r.present == (ADSB_ES_HAS_EMERGENCY | ADSB_ES_HAS_SQUAWK) && r.half[0] <= 7777 && r.half[0] % 10 <= 7 &&
              r.half[0] / 10 % 10 <= 7 && r.half[0] / 100 % 10 <= 7 && r.value == 0 && r.half[1] == 0);
        break;
    case ADSB_ES_ACAS_RA:
        CHECK(r.present == ADSB_ES_HAS_RA && r.half[1] == 0 && r.flags == 0);
        break;
    case ADSB_ES_TARGET_STATE:
        CHECK(r.version == 2 && (r.present & ADSB_ES_HAS_VERSION) && r.value <= 65472 && r.value % 32 == 0 && r.half[1] < 512);
        CHECK(r.present & ADSB_ES_HAS_BARO ? r.half[0] >= 8000 && r.half[0] <= 12080 && r.half[0] % 8 == 0 : r.half[0] == 0);
        CHECK((r.present & ADSB_ES_HAS_MODES) ||
              (r.flags & (ADSB_ES_AUTOPILOT | ADSB_ES_VNAV | ADSB_ES_ALT_HOLD | ADSB_ES_APPROACH | ADSB_ES_LNAV)) == 0);
        break;
    case ADSB_ES_OPERATIONAL:
        CHECK((r.present & ADSB_ES_HAS_VERSION) && r.value == 0 && st <= 1);
        if (r.version >= 3) CHECK(r.present == ADSB_ES_HAS_VERSION && r.half[0] == 0 && r.half[1] == 0 && r.flags == 0);
        if (r.version <= 1) CHECK((r.present & (ADSB_ES_HAS_SIL_SUPPLEMENT | ADSB_ES_HAS_SDA | ADSB_ES_HAS_GVA | ADSB_ES_HAS_NIC_C | ADSB_ES_HAS_NAC_V)) == 0);
        if (r.version == 0) CHECK(r.present == (ADSB_ES_HAS_VERSION | ADSB_ES_HAS_CC_OM));
        break;
    default:
        CHECK(r.state == ADSB_ES_RESERVED && r.present == 0 && r.flags == 0 && r.value == 0 && r.half[0] == 0 && r.half[1] == 0);
    }
}

// one list on exact-size heap copies, twice
static void run(const std::vector<adsb_frame> &list)
{
    const size_t n = list.size();
    adsb_frame *fr = static_cast<adsb_frame *>(std::malloc(n ? sizeof(adsb_frame) * n : 1));
    adsb_es_rec *recs = static_cast<adsb_es_rec *>(std::malloc(n ? sizeof(adsb_es_rec) * n : 1));
    adsb_es_rec *again = static_cast<adsb_es_rec *>(std::malloc(n ? sizeof(adsb_es_rec) * n : 1));
    adsb_es_header *h = static_cast<adsb_es_header *>(std::malloc(sizeof(adsb_es_header)));
    if (n) std::memcpy(fr, list.data(), sizeof(adsb_frame) * n);
    std::memset(recs, 0xEE, n ? sizeof(adsb_es_rec) * n : 1);
    std::memset(again, 0x11, n ? sizeof(adsb_es_rec) * n : 1);
    std::memset(h, 0xEE, sizeof(*h));
    CHECK(adsb_host_es(fr, n, recs, h) == ADSB_OK);
    CHECK(adsb_host_es(fr, n, again, nullptr) == ADSB_OK && adsb_host_es(fr, n, nullptr, nullptr) == ADSB_OK);
    CHECK(n == 0 || std::memcmp(recs, again, sizeof(adsb_es_rec) * n) == 0); // every byte written, the same twice
    uint64_t states[ADSB_ES_STATES] = {}, versions[4] = {};
    for (size_t j = 0; j < n; ++j) {
        check_record(fr[j], recs[j]);
        if (recs[j].state < ADSB_ES_STATES) states[recs[j].state] += 1;
        if (recs[j].state == ADSB_ES_OPERATIONAL) versions[recs[j].version < 3 ? recs[j].version : 3] += 1;
    }
    n_frames += n;
    CHECK(h->n == n && h->reserved == 0);
    for (unsigned k = 0; k < ADSB_ES_STATES; ++k) CHECK(h->n_state[k] == states[k]);
    for (unsigned k = 0; k < 4; ++k) CHECK(h->n_version[k] == versions[k]);
    std::free(h);
    std::free(again);
    std::free(recs);
    std::free(fr);
}

static const unsigned kReadTypeCodes[4] = {19, 28, 29, 31};
static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

int main()
{
    std::vector<adsb_frame> list;
    run(list); // n = 0, with and without arrays
    CHECK(adsb_host_es(nullptr, 0, nullptr, nullptr) == ADSB_OK && adsb_host_es(nullptr, 1, nullptr, nullptr) == ADSB_E_ARG);

    // every first byte over payloads of every state
    const uint64_t rest = (1ull << 48) - 1;
    const uint64_t some[] = {tc_st(4, 3) | 0x2CC371C32CE0ull, tc_st(11, 1) | rest, tc_st(19, 1) | rest, tc_st(28, 1) | rest, tc_st(28, 2) | rest,
                             tc_st(29, 2) | rest, tc_st(31, 0) | rest, tc_st(31, 1) | (rest & ~field(41, 3, 5)), tc_st(23, 0), 0};
    for (unsigned df = 0; df < 32; ++df)
        for (unsigned low3 = 0; low3 < 8; ++low3)
            for (uint64_t me : some) list.push_back(frame_of(me, df, low3));
    run(list);
    list.clear();

    // every type code with every subtype: the payload empty, full, every single bit and every pair of bits
    for (unsigned tc = 0; tc < 32; ++tc)
        for (unsigned st = 0; st < 8; ++st) {
            list.push_back(frame_of(tc_st(tc, st)));
            list.push_back(frame_of(tc_st(tc, st) | rest, 18, st & 1));
            const bool read = tc == 19 || tc == 28 || tc == 29 || tc == 31;
            for (unsigned a = 9; a <= 56; ++a) {
                list.push_back(frame_of(tc_st(tc, st) | bit(a)));
                list.push_back(frame_of((tc_st(tc, st) | rest) & ~bit(a)));
                if (read && st < 4)
                    for (unsigned b = a + 1; b <= 56; ++b) list.push_back(frame_of(tc_st(tc, st) | bit(a) | bit(b)));
            }
        }
    run(list);
    list.clear();

    // every squawk field with every emergency state; every altitude, setting and heading of a target state; every
    // version with every supplement and category bit pattern of an operational status
    for (unsigned f = 0; f < (1u << 13); ++f) list.push_back(frame_of(tc_st(28, 1) | field(9, 3, f) | field(12, 13, f)));
    for (unsigned n = 0; n < 2048; ++n)
        list.push_back(frame_of(tc_st(29, 2 | (n & 1)) | field(10, 11, n) | field(21, 9, n) | field(30, 10, n) | field(47, 8, n)));
    for (unsigned v = 0; v < 8; ++v)
        for (unsigned x = 0; x < 8192; ++x)
            list.push_back(frame_of(tc_st(31, x & 1) | field(41, 3, v) | field(44, 13, x) | field(17, 16, x * 5u)));
    run(list);
    list.clear();

    // random frames: uniform bytes, and extended squitters with random payloads
    for (int round = 0; round < 6; ++round) {
        for (int j = 0; j < 50000; ++j) {
            adsb_frame f = frame_of(rnd() >> 8, j % 3 ? 17 + j % 2 : (unsigned)(rnd() % 32), (unsigned)(rnd() % 8));
            if (j % 5 == 0) f.bytes[4] = (uint8_t)(kReadTypeCodes[rnd() % 4] << 3 | rnd() % 8);
            list.push_back(f);
        }
        run(list);
        list.clear();
    }

    // the integrity function: every type code, version and supplement set, values far outside them, NULL outputs
    unsigned long n_integrity = 0;
    for (uint32_t tc : {0u, 1u, 4u, 5u, 6u, 7u, 8u, 9u, 10u, 11u, 12u, 13u, 14u, 15u, 16u, 17u, 18u, 19u, 20u, 21u, 22u, 23u, 28u, 29u, 31u, 32u, 255u, 0x80000000u, 0xFFFFFFFFu})
        for (uint32_t version : {0u, 1u, 2u, 3u, 7u, 8u, (uint32_t)ADSB_ES_VERSION_UNKNOWN, 0x100u, 0x80000000u, 0xFFFFFFFFu})
            for (uint32_t supp : {0u, 1u, 2u, 3u, 4u, 5u, 6u, 7u, 8u, 0xFFFFFFF8u, 0xFFFFFFFFu}) {
                uint32_t nic = 99, rc = 99, nic2 = 98, rc2 = 98;
                CHECK(adsb_host_es_integrity(tc, version, supp, &nic, &rc) == ADSB_OK && nic <= 11 && (rc == 0 || rc_of_the_table(rc)));
                CHECK(adsb_host_es_integrity(tc, version, supp & 7u, &nic2, &rc2) == ADSB_OK && nic2 == nic && rc2 == rc); // bits 0-2 only
                CHECK(adsb_host_es_integrity(tc, version, supp, nullptr, &rc2) == ADSB_OK && adsb_host_es_integrity(tc, version, supp, &nic2, nullptr) == ADSB_OK);
                CHECK(adsb_host_es_integrity(tc, version, supp, nullptr, nullptr) == ADSB_OK);
                if (version == 0 || version == ADSB_ES_VERSION_UNKNOWN) CHECK(nic == 0);
                if (tc > 22 || tc == 19 || (tc >= 1 && tc <= 4)) CHECK(nic == 0 && rc == 0);
                ++n_integrity;
            }

    for (unsigned k = 0; k < ADSB_ES_STATES; ++k) CHECK(n_state[k] > 0);
    std::printf("es_edges: %lu frames (", n_frames);
    for (unsigned k = 0; k < ADSB_ES_STATES; ++k) std::printf("%s%lu", k ? ", " : "", n_state[k]);
    std::printf(" per state), %lu integrity calls, %d failures\n", n_integrity, fails);
    return fails ? 1 : 0;
}
