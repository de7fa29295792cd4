// commb_edges.cpp -- stand-alone sanitizer run of the CPU mirror of the Comm-B stage (adsb_host_commb and
// adsb_host_commb_as, air_rs_amd/csrc/host/adsb_commb.cpp, which compiles the text the device compiles:
// air_rs_amd/csrc/adsb_commb.h).  Exact-size heap buffers for the frames in and the records out, so that a read or
// write beside them is a heap-buffer-overflow; every single bit and every pair of bits of MB, every status bit cleared
// over every bit of its field, every field of 4,0 / 5,0 / 6,0 at its minimum, its maximum and the values around each
// limit (the sign bit alone among them: s = -2^n, whose negation must not overflow), every reserved bit, every DF,
// every register code 0..255 and a few wide ones through commb_as, and a few hundred thousand random payloads.  What
// holds whatever the input is checked on every record.  Host sources only, no device:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/host/commb_edges.cpp
//       air_rs_amd/csrc/host/adsb_commb.cpp -o /tmp/commb_edges && /tmp/commb_edges   (one command)
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

static unsigned long n_frames = 0, n_as = 0, n_state[5] = {0, 0, 0, 0, 0};
static const uint32_t kCodes[7] = {0x10, 0x17, 0x20, 0x30, 0x40, 0x50, 0x60};

static adsb_frame frame_of(uint64_t mb, unsigned df = 20)
{
    adsb_frame f;
    std::memset(&f, 0xA5, sizeof(f));
    f.bytes[0] = (uint8_t)(df << 3 | 5);
    for (int k = 0; k < 7; ++k) f.bytes[4 + k] = (uint8_t)(mb >> (48 - 8 * k));
    return f;
}

// bit a (1..56) of MB as a mask of the 56-bit number
static uint64_t bit(unsigned a) { return 1ull << (56 - a); }
// the n bits from bit a set to x
static uint64_t field(unsigned a, unsigned n, uint64_t x) { return (x & ((1ull << n) - 1)) << (57 - a - n); }

// the invariants of one record, whatever the frame
static void check_record(const adsb_frame &f, const adsb_commb_rec &r)
{
    const unsigned df = f.bytes[0] >> 3;
    CHECK(r.state <= ADSB_COMMB_AMBIGUOUS && r.reserved == 0);
    n_state[r.state <= 4 ? r.state : 0] += 1;
    unsigned bits = 0;
    for (int k = 0; k < 7; ++k) bits += r.candidates >> k & 1;
    CHECK(r.n_candidates == bits && r.candidates < 0x80);
    bool zero_mb = true;
    for (int k = 4; k < 11; ++k) zero_mb = zero_mb && f.bytes[k] == 0;
    if (df != 20 && df != 21) CHECK(r.state == ADSB_COMMB_NOT_COMMB);
    else if (zero_mb) CHECK(r.state == ADSB_COMMB_EMPTY);
    else CHECK(r.state == (bits == 0 ? ADSB_COMMB_NONE : bits == 1 ? ADSB_COMMB_ONE : ADSB_COMMB_AMBIGUOUS));
    if (r.state != ADSB_COMMB_ONE) {
        CHECK(r.bds == 0 && r.status == 0 && r.word == 0);
        for (int k = 0; k < 5; ++k) CHECK(r.value[k] == 0);
        if (r.state < ADSB_COMMB_NONE) CHECK(r.candidates == 0);
    }
}

static void check_one(const adsb_commb_rec &r)
{
    CHECK(r.state == ADSB_COMMB_ONE && r.status < 0x20);
    for (int k = 0; k < 5; ++k)
        if (!(r.status >> k & 1)) CHECK(r.value[k] == 0);
    switch (r.bds) {
    case 0x40:
        CHECK(r.word == 0 && r.value[0] >= 0 && r.value[0] <= 16 * 4095 && r.value[1] >= 0 && r.value[1] <= 16 * 4095);
        CHECK((!(r.status & 4) || (r.value[2] >= 8000 && r.value[2] <= 12095)) && r.value[3] >= 0 && r.value[3] <= 7 && r.value[4] >= 0 && r.value[4] <= 3);
        break;
    case 0x50:
        CHECK(r.word == 0 && r.value[0] >= -284 && r.value[0] <= 284 && r.value[1] >= 0 && r.value[1] <= 2047);
        CHECK(r.value[2] >= 0 && r.value[2] <= 600 && r.value[3] >= -512 && r.value[3] <= 511 && r.value[4] >= 0 && r.value[4] <= 500);
        break;
    case 0x60:
        CHECK(r.word == 0 && r.value[0] >= 0 && r.value[0] <= 2047 && r.value[1] >= 0 && r.value[1] <= 500 && r.value[2] >= 0 && r.value[2] <= 250);
        CHECK(r.value[3] >= -5984 && r.value[3] <= 5984 && r.value[4] >= -5984 && r.value[4] <= 5984 && r.value[3] % 32 == 0 && r.value[4] % 32 == 0);
        break;
    case 0x30:
        CHECK(r.status == 0x1F && r.word >> 24 == 0x30 && r.value[3] != 3 && (r.value[0] & 0x7F) < 48);
        break;
    case 0x10:
        CHECK(r.status == 0x3 && r.word >> 24 == 0x10 && (r.value[1] ? r.value[0] >= 5 : r.value[0] <= 4) && r.value[0] <= 127);
        break;
    case 0x17:
        CHECK(r.status == 0 && r.word < (1u << 28) && (r.word >> 21 & 1));
        break;
    case 0x20:
        CHECK(r.status == 0 && r.word == 0);
        break;
    default:
        CHECK(!"a register that is none of the seven");
    }
}

// one list on exact-size heap copies, twice; then every register code through commb_as for each frame
static void run(const std::vector<adsb_frame> &list)
{
    const size_t n = list.size();
    adsb_frame *fr = static_cast<adsb_frame *>(std::malloc(n ? sizeof(adsb_frame) * n : 1));
    adsb_commb_rec *recs = static_cast<adsb_commb_rec *>(std::malloc(n ? sizeof(adsb_commb_rec) * n : 1));
    adsb_commb_rec *again = static_cast<adsb_commb_rec *>(std::malloc(n ? sizeof(adsb_commb_rec) * n : 1));
    adsb_commb_header *h = static_cast<adsb_commb_header *>(std::malloc(sizeof(adsb_commb_header)));
    if (n) std::memcpy(fr, list.data(), sizeof(adsb_frame) * n);
    std::memset(recs, 0xEE, n ? sizeof(adsb_commb_rec) * n : 1);
    std::memset(again, 0x11, n ? sizeof(adsb_commb_rec) * n : 1);
    std::memset(h, 0xEE, sizeof(*h));
    CHECK(adsb_host_commb(fr, n, recs, h) == ADSB_OK);
    CHECK(adsb_host_commb(fr, n, again, nullptr) == ADSB_OK && adsb_host_commb(fr, n, nullptr, nullptr) == ADSB_OK);
    CHECK(n == 0 || std::memcmp(recs, again, sizeof(adsb_commb_rec) * n) == 0); // every byte written, the same twice
    uint64_t states[5] = {0, 0, 0, 0, 0}, regs[7] = {0, 0, 0, 0, 0, 0, 0};
    for (size_t j = 0; j < n; ++j) {
        const adsb_commb_rec &r = recs[j];
        check_record(fr[j], r);
        if (r.state <= 4) states[r.state] += 1;
        if (r.state == ADSB_COMMB_ONE) check_one(r);
        uint8_t *bytes = static_cast<uint8_t *>(std::malloc(14));
        adsb_commb_rec *as = static_cast<adsb_commb_rec *>(std::malloc(sizeof(adsb_commb_rec)));
        std::memcpy(bytes, fr[j].bytes, 14);
        for (int k = 0; k < 7; ++k) {
            std::memset(as, 0xEE, sizeof(*as));
            const int rc = adsb_host_commb_as(bytes, kCodes[k], as);
            ++n_as;
            if (r.candidates >> k & 1) {
                CHECK(rc == ADSB_OK && as->bds == kCodes[k] && as->candidates == r.candidates && as->n_candidates == r.n_candidates);
                check_one(*as);
                if (r.state == ADSB_COMMB_ONE) {
                    CHECK(std::memcmp(as, &r, sizeof(r)) == 0);
                    regs[k] += 1;
                }
            } else {
                CHECK(rc == ADSB_E_ARG && as->state == 0xEE && as->word == 0xEEEEEEEEu);
            }
        }
        std::free(as);
        std::free(bytes);
    }
    n_frames += n;
    CHECK(h->n == n && h->n_commb == n - states[0] && h->n_empty == states[1] && h->n_none == states[2] && h->n_one == states[3] &&
          h->n_ambiguous == states[4] && h->reserved[0] == 0 && h->reserved[1] == 0 && h->reserved[2] == 0);
    for (int k = 0; k < 7; ++k) CHECK(h->n_bds[k] == regs[k]);
    std::free(h);
    std::free(again);
    std::free(recs);
    std::free(fr);
}

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
    CHECK(adsb_host_commb(nullptr, 0, nullptr, nullptr) == ADSB_OK && adsb_host_commb(nullptr, 1, nullptr, nullptr) == ADSB_E_ARG);

    // every single bit, every pair of bits, all ones, under DF20 and DF21
    list.push_back(frame_of(0));
    list.push_back(frame_of((1ull << 56) - 1, 21));
    for (unsigned a = 1; a <= 56; ++a) {
        list.push_back(frame_of(bit(a), 20 + a % 2));
        list.push_back(frame_of(((1ull << 56) - 1) & ~bit(a)));
        for (unsigned b = a + 1; b <= 56; ++b) list.push_back(frame_of(bit(a) | bit(b)));
    }
    run(list);
    list.clear();

    // every DF with payloads of every register
    const uint64_t full40 = bit(1) | field(2, 12, 0x555) | bit(14) | field(15, 12, 0x2AA) | bit(27) | field(28, 12, 0x333) | bit(48) | field(49, 3, 5) | bit(54) | field(55, 2, 2);
    const uint64_t full50 = bit(1) | field(2, 10, (uint64_t)-100) | bit(12) | field(13, 11, (uint64_t)-300) | bit(24) | field(25, 10, 220) | bit(35) | field(36, 10, (uint64_t)-7) | bit(46) | field(47, 10, 230);
    const uint64_t full60 = bit(1) | field(2, 11, (uint64_t)-400) | bit(13) | field(14, 10, 280) | bit(24) | field(25, 10, 200) | bit(35) | field(36, 10, (uint64_t)-60) | bit(46) | field(47, 10, 55);
    const uint64_t some[] = {full40, full50, full60, field(1, 8, 0x10) | field(17, 7, 3), field(1, 8, 0x10) | bit(15) | field(17, 7, 127) | 0xFFFFFFFFull,
                             bit(7) | bit(1) | bit(24), field(1, 28, 0xFFFFFFF), field(1, 8, 0x20) | field(9, 48, 0x2CC371C31DE0ull),
                             field(1, 8, 0x30) | field(9, 14, 0x2A85) | field(31, 26, 0x3FFFFFF), field(1, 8, 0x30) | field(29, 2, 3)};
    for (unsigned df = 0; df < 32; ++df)
        for (uint64_t mb : some) list.push_back(frame_of(mb, df));
    run(list);
    list.clear();

    // a status bit cleared over every bit of its field, and over the whole field
    struct Guard { uint64_t full; unsigned a, first, n; };
    const Guard guards[] = {{full40, 1, 2, 12}, {full40, 14, 15, 12}, {full40, 27, 28, 12}, {full40, 48, 49, 3}, {full40, 54, 55, 2},
                            {full50, 1, 2, 10}, {full50, 12, 13, 11}, {full50, 24, 25, 10}, {full50, 35, 36, 10}, {full50, 46, 47, 10},
                            {full60, 1, 2, 11}, {full60, 13, 14, 10}, {full60, 24, 25, 10}, {full60, 35, 36, 10}, {full60, 46, 47, 10}};
    for (const Guard &g : guards) {
        const uint64_t base = g.full & ~bit(g.a) & ~field(g.first, g.n, ~0ull);
        list.push_back(frame_of(base));
        list.push_back(frame_of(base | field(g.first, g.n, ~0ull)));
        for (unsigned x = g.first; x < g.first + g.n; ++x) list.push_back(frame_of(base | bit(x)));
        // ... and with the status bit set: the field at its ends, the sign bit alone, and around every limit
        for (int64_t v : {0, 1, 47, 48, 100, 101, 187, 188, 250, 251, 284, 285, 300, 301, 500, 501, 511, 512, 1023, 1024, 2047, 4095,
                          -1, -187, -188, -284, -285, -512, -1024, -2048})
            list.push_back(frame_of(base | bit(g.a) | field(g.first, g.n, (uint64_t)v)));
    }
    // the two speeds of 5,0 around their largest difference
    for (int gs : {0, 100, 149, 150, 151, 200, 300})
        for (int tas : {0, 99, 100, 101, 200, 250})
            list.push_back(frame_of(bit(24) | field(25, 10, (uint64_t)gs) | bit(46) | field(47, 10, (uint64_t)tas)));
    // every reserved bit of 1,0 / 1,7 / 4,0; every version with both overlay bits
    for (unsigned a = 10; a <= 14; ++a) list.push_back(frame_of(some[3] | bit(a)));
    for (unsigned a = 29; a <= 56; ++a) list.push_back(frame_of(some[5] | bit(a)));
    for (unsigned a : {40u, 41u, 42u, 43u, 44u, 45u, 46u, 47u, 52u, 53u}) list.push_back(frame_of(full40 | bit(a)));
    for (unsigned v = 0; v < 128; ++v)
        for (unsigned ovc = 0; ovc < 2; ++ovc) list.push_back(frame_of(field(1, 8, 0x10) | field(15, 1, ovc) | field(17, 7, v)));
    // every character value in every place of 2,0; every u(16,7) and TTI of 3,0
    for (unsigned k = 0; k < 8; ++k)
        for (unsigned c = 0; c < 64; ++c) list.push_back(frame_of(field(1, 8, 0x20) | field(9, 48, 0x2CC371C31DE0ull & ~(0x3Full << (42 - 6 * k))) | field(9 + 6 * k, 6, c)));
    for (unsigned v = 0; v < 128; ++v)
        for (unsigned tti = 0; tti < 4; ++tti) list.push_back(frame_of(field(1, 8, 0x30) | field(16, 7, v) | field(29, 2, tti)));
    run(list);
    list.clear();

    // random payloads: uniform, and the registers' full payloads with a few random bits turned
    for (int round = 0; round < 6; ++round) {
        for (int j = 0; j < 50000; ++j) {
            uint64_t mb = rnd() >> 8;
            if (j % 4) {
                mb = some[rnd() % (sizeof(some) / sizeof(some[0]))];
                for (int flips = (int)(rnd() % 4); flips > 0; --flips) mb ^= bit(1 + (unsigned)(rnd() % 56));
            }
            list.push_back(frame_of(mb, j % 9 ? 20 + j % 2 : (unsigned)(rnd() % 32)));
        }
        run(list);
        list.clear();
    }

    // commb_as: every code 0..255 and a few wide ones on an ambiguous payload, NULL arguments
    {
        adsb_frame f = frame_of(bit(24) | field(25, 10, 250)); // 5,0 and 6,0
        adsb_commb_rec r;
        for (uint32_t code = 0; code < 256; ++code) {
            const int rc = adsb_host_commb_as(f.bytes, code, &r);
            CHECK(rc == (code == 0x50 || code == 0x60 ? ADSB_OK : ADSB_E_ARG));
            if (rc == ADSB_OK) CHECK(r.bds == code && r.status == 0x4 && r.value[2] == (code == 0x50 ? 500 : 250));
        }
        for (uint32_t code : {0x100u, 0x150u, 0x1050u, 0x80000050u, 0xFFFFFFFFu, 0x500u, 0x5000u})
            CHECK(adsb_host_commb_as(f.bytes, code, &r) == ADSB_E_ARG);
        CHECK(adsb_host_commb_as(nullptr, 0x50, &r) == ADSB_E_ARG && adsb_host_commb_as(f.bytes, 0x50, nullptr) == ADSB_E_ARG);
    }

    CHECK(n_state[0] && n_state[1] && n_state[2] && n_state[3] && n_state[4]);
    std::printf("commb_edges: %lu frames (%lu not Comm-B, %lu empty, %lu none, %lu one, %lu ambiguous), %lu commb_as calls, %d failures\n",
                n_frames, n_state[0], n_state[1], n_state[2], n_state[3], n_state[4], n_as, fails);
    return fails ? 1 : 0;
}
