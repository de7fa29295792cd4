// modes_edges.cpp -- stand-alone sanitizer run of the CPU mirror of the Mode S stage (adsb_host_modes,
// air_rs_amd/csrc/host/adsb_modes.cpp over air_rs_amd/csrc/adsb_modes.h, the text the device compiles too) and of the
// wire input with ADSB_WIRE_IN_SHORT (adsb_host_wire_parse): the pieces of the feature that read and write caller memory
// on the CPU.  Exact-size heap buffers, so that one frame read past the list, one record, address or squitter written
// past its room, or one byte read past a stream's end is a heap-buffer-overflow: lists of every kind of frame with
// known_in empty, of one and holding the list's addresses; every cut of a list with the known set carried over; every
// optional output left out; streams of short frames cut at every length, with every `max` from 0 to one past the frames
// that exist.  Host sources only, no device:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/host/modes_edges.cpp \
//       air_rs_amd/csrc/host/adsb_modes.cpp air_rs_amd/csrc/host/adsb_wire_in.cpp -o /tmp/modes_edges && /tmp/modes_edges
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

static uint32_t crc24(const uint8_t *d, size_t n)
{
    uint32_t r = 0;
    for (size_t b = 0; b < n; ++b)
        for (int i = 7; i >= 0; --i) {
            const uint32_t feed = ((r >> 23) ^ (d[b] >> i)) & 1u;
            r = (r << 1) & 0xFFFFFFu;
            if (feed) r ^= 0xFFF409u;
        }
    return r;
}

// head (4 bytes) + for a long DF 7 more, then crc ^ word: word 0 checks itself, an address is address/parity
static adsb_frame frame_of(uint8_t df, uint8_t low3, uint32_t aa_or_fields, uint32_t word, uint8_t fill, uint64_t offset)
{
    adsb_frame f;
    std::memset(&f, 0, sizeof(f));
    f.offset = offset;
    f.fixed_bit = 0xFF;
    f.bytes[0] = (uint8_t)(df << 3 | low3);
    f.bytes[1] = (uint8_t)(aa_or_fields >> 16), f.bytes[2] = (uint8_t)(aa_or_fields >> 8), f.bytes[3] = (uint8_t)aa_or_fields;
    const size_t payload = df < 16 ? 4 : 11;
    for (size_t k = 4; k < payload; ++k) f.bytes[k] = (uint8_t)(fill + 7 * k);
    if (df >= 20 && df <= 21 && (fill & 1)) f.bytes[4] = 0x20;
    const uint32_t p = crc24(f.bytes, payload) ^ word;
    f.bytes[payload] = (uint8_t)(p >> 16), f.bytes[payload + 1] = (uint8_t)(p >> 8), f.bytes[payload + 2] = (uint8_t)p;
    return f;
}

struct Result {
    std::vector<adsb_modes_rec> recs;
    std::vector<uint32_t> known;
    std::vector<adsb_frame> squitters;
    std::vector<uint64_t> sq_counts;
    adsb_modes_header h;
};

// One call with every buffer at its exact size
static Result run(const std::vector<adsb_frame> &list, const std::vector<uint32_t> &known_in, const std::vector<uint64_t> &counts)
{
    const size_t n = list.size(), nk = known_in.size(), R = counts.size();
    adsb_frame *fr = static_cast<adsb_frame *>(std::malloc(n ? n * sizeof(adsb_frame) : 1));
    if (n) std::memcpy(fr, list.data(), n * sizeof(adsb_frame));
    uint32_t *ki = static_cast<uint32_t *>(std::malloc(nk ? nk * 4 : 1));
    if (nk) std::memcpy(ki, known_in.data(), nk * 4);
    uint64_t *cn = static_cast<uint64_t *>(std::malloc(R ? R * 8 : 1));
    if (R) std::memcpy(cn, counts.data(), R * 8);
    adsb_modes_rec *recs = static_cast<adsb_modes_rec *>(std::malloc(n ? n * sizeof(adsb_modes_rec) : 1));
    uint32_t *ko = static_cast<uint32_t *>(std::malloc(n + nk ? (n + nk) * 4 : 1));
    adsb_frame *sq = static_cast<adsb_frame *>(std::malloc(n ? n * sizeof(adsb_frame) : 1));
    uint64_t *sc = static_cast<uint64_t *>(std::malloc(R ? R * 8 : 1));
    Result r;
    CHECK(adsb_host_modes(n ? fr : nullptr, n, R ? cn : nullptr, (uint32_t)R, nk ? ki : nullptr, nk, recs, ko, sq, sc, &r.h) == ADSB_OK);
    CHECK(r.h.n == n && r.h.n_self + r.h.n_known + r.h.n_unknown + r.h.n_parity + r.h.n_unsupported == n);
    CHECK(r.h.n_known_out <= n + nk && r.h.n_known_out >= nk && r.h.n_squitters <= r.h.n_self);
    r.recs.assign(recs, recs + n);
    r.known.assign(ko, ko + r.h.n_known_out);
    r.squitters.assign(sq, sq + r.h.n_squitters);
    r.sq_counts.assign(sc, sc + R);
    for (size_t k = 1; k < r.known.size(); ++k) CHECK(r.known[k - 1] < r.known[k]);
    uint64_t sum = 0;
    for (uint64_t c : r.sq_counts) sum += c;
    CHECK(!R || sum == r.h.n_squitters);
    // every optional output left out: the header alone, and nothing at all
    adsb_modes_header h2;
    CHECK(adsb_host_modes(n ? fr : nullptr, n, nullptr, 0, nk ? ki : nullptr, nk, nullptr, nullptr, nullptr, nullptr, &h2) == ADSB_OK);
    CHECK(std::memcmp(&h2, &r.h, sizeof(h2)) == 0);
    CHECK(adsb_host_modes(n ? fr : nullptr, n, nullptr, 0, nk ? ki : nullptr, nk, nullptr, nullptr, nullptr, nullptr, nullptr) == ADSB_OK);
    std::free(sc), std::free(sq), std::free(ko), std::free(recs), std::free(cn), std::free(ki), std::free(fr);
    return r;
}

static std::vector<adsb_frame> mixed(size_t n)
{
    static const uint8_t dfs[] = {17, 11, 4, 5, 20, 21, 0, 16, 18, 24, 31, 1, 19, 11, 17, 4};
    static const uint32_t pool[] = {0x000000, 0xFFFFFF, 0x4840D6, 0xABCDEF, 0x3C6614};
    std::vector<adsb_frame> out;
    uint32_t x = 12345;
    for (size_t i = 0; i < n; ++i) {
        x = x * 1664525u + 1013904223u;
        const uint8_t df = dfs[(x >> 8) % 16];
        const uint32_t a = pool[(x >> 16) % 5];
        const bool self = df == 17 || df == 18 || df == 11;
        const uint32_t word = self ? ((x >> 24) % 4 == 0 ? (x >> 4) % 200 : 0) : ((x >> 24) % 5 == 0 ? x & 0xFFFFFF : a);
        out.push_back(frame_of(df, (uint8_t)(x & 7), self ? a : x >> 3, word, (uint8_t)(x >> 12), 100 * i));
    }
    return out;
}

static void wire_short()
{
    // a Beast stream of '1', '2' and '3' frames with doubled 0x1A bytes, and an AVR text of all six shapes
    std::vector<uint8_t> beast, avr;
    const adsb_frame s = frame_of(11, 5, 0x1A1A1A, 0, 0, 0), l = frame_of(17, 5, 0x4840D6, 0, 3, 0);
    auto put = [&](uint8_t v) { beast.push_back(v); if (v == 0x1A) beast.push_back(v); };
    for (int k = 0; k < 9; ++k) {
        const int len = k % 3 == 0 ? 7 : k % 3 == 1 ? 14 : 2;
        beast.push_back(0x1A), beast.push_back(len == 7 ? '2' : len == 14 ? '3' : '1');
        for (int t = 0; t < 6; ++t) put(t == 5 ? (uint8_t)k : t == 2 ? 0x1A : 0);
        put(k & 1 ? 0x1A : 0x40);
        for (int b = 0; b < len; ++b) put(len == 7 ? s.bytes[b] : l.bytes[b]);
        char line[64];
        int at = std::snprintf(line, sizeof(line), "%s", k & 1 ? "@0000001A2B3C" : "*");
        for (int b = 0; b < len; ++b) at += std::snprintf(line + at, sizeof(line) - at, k & 2 ? "%02x" : "%02X", len == 7 ? s.bytes[b] : l.bytes[b]);
        std::snprintf(line + at, sizeof(line) - at, ";\n");
        avr.insert(avr.end(), line, line + std::strlen(line));
    }
    for (int pass = 0; pass < 2; ++pass) {
        const std::vector<uint8_t> &in = pass ? avr : beast;
        for (uint32_t filter : {ADSB_WIRE_IN_SHORT, ADSB_WIRE_IN_SHORT | ADSB_WIRE_IN_CRC, ADSB_WIRE_IN_SHORT | ADSB_WIRE_IN_DF17, 0u}) {
            adsb_wire_in_cfg cfg = {pass ? ADSB_WIRE_AVR : ADSB_WIRE_BEAST, filter, 0, 0, ADSB_SAMPLE_I8, 1};
            uint64_t whole_frames = 0;
            for (size_t c = 0; c <= in.size(); ++c) { // every prefix, its buffers exactly as large as max_frames = 0 promises
                const size_t max = c / (filter & ADSB_WIRE_IN_SHORT ? 16 : 23);
                uint8_t *bytes = static_cast<uint8_t *>(std::malloc(c ? c : 1));
                if (c) std::memcpy(bytes, in.data(), c);
                adsb_frame *fr = static_cast<adsb_frame *>(std::malloc(max ? max * sizeof(adsb_frame) : 1));
                adsb_wire_rx *rx = static_cast<adsb_wire_rx *>(std::malloc(max ? max * sizeof(adsb_wire_rx) : 1));
                adsb_frame_level *lv = static_cast<adsb_frame_level *>(std::malloc(max ? max * sizeof(adsb_frame_level) : 1));
                uint64_t end = c, counts = 0, consumed = 0;
                size_t got = 0;
                adsb_wire_in_header h;
                CHECK(adsb_host_wire_parse(&cfg, c ? bytes : nullptr, c, &end, 1, fr, rx, lv, max, &got, &counts, &consumed, &h) == ADSB_OK);
                CHECK(h.flags == 0 && got == h.n_frames && h.n_frames == h.total_found && consumed <= c && c - consumed <= 43);
                for (size_t i = 0; i < got; ++i) {
                    const bool is_short = rx[i].kind == '2' || (pass && fr[i].bytes[0] >> 3 < 16);
                    CHECK(!is_short || std::memcmp(fr[i].bytes + 7, "\0\0\0\0\0\0\0", 7) == 0);
                    CHECK((filter & ADSB_WIRE_IN_SHORT) || !is_short);
                }
                whole_frames = h.n_frames;
                std::free(lv), std::free(rx), std::free(fr), std::free(bytes);
            }
            CHECK(whole_frames == (filter == ADSB_WIRE_IN_SHORT ? 6u : filter == 0u ? 3u : filter & ADSB_WIRE_IN_CRC ? 6u : 3u));
            for (size_t max = 0; max <= 7; ++max) { // output room from none to one more than needed
                adsb_frame *fr = static_cast<adsb_frame *>(std::malloc(max ? max * sizeof(adsb_frame) : 1));
                uint64_t end = in.size();
                size_t got = 0;
                CHECK(adsb_host_wire_parse(&cfg, in.data(), in.size(), &end, 1, fr, nullptr, nullptr, max, &got, nullptr, nullptr, nullptr) == ADSB_OK);
                CHECK(got == (max < whole_frames ? max : whole_frames));
                std::free(fr);
            }
        }
        std::printf("%s with short frames: %zu bytes, every prefix, four filters\n", pass ? "avr" : "beast", in.size());
    }
}

int main()
{
    const std::vector<adsb_frame> list = mixed(200);
    const std::vector<uint32_t> none, one = {0x4840D6}, all = {0x000000, 0x3C6614, 0x4840D6, 0xABCDEF, 0xFFFFFF};
    for (const std::vector<uint32_t> &known : {none, one, all}) {
        const Result whole = run(list, known, {50, 0, 150});
        std::printf("200 frames, %zu known: self %llu known %llu unknown %llu parity %llu unsupported %llu, known_out %llu, squitters %llu\n",
                    known.size(), (unsigned long long)whole.h.n_self, (unsigned long long)whole.h.n_known,
                    (unsigned long long)whole.h.n_unknown, (unsigned long long)whole.h.n_parity,
                    (unsigned long long)whole.h.n_unsupported, (unsigned long long)whole.h.n_known_out,
                    (unsigned long long)whole.h.n_squitters);
        CHECK(whole.h.n_self && whole.h.n_known && whole.h.n_unknown && whole.h.n_parity && whole.h.n_unsupported);
        for (size_t cut = 0; cut <= list.size(); ++cut) { // the cut property, the known set carried over
            const Result a = run(std::vector<adsb_frame>(list.begin(), list.begin() + cut), known, {});
            const Result b = run(std::vector<adsb_frame>(list.begin() + cut, list.end()), a.known, {list.size() - cut});
            CHECK(b.known == whole.known && a.squitters.size() + b.squitters.size() == whole.squitters.size());
            CHECK(cut == 0 || std::memcmp(a.recs.data(), whole.recs.data(), cut * sizeof(adsb_modes_rec)) == 0);
            CHECK(cut == list.size() ||
                  std::memcmp(b.recs.data(), whole.recs.data() + cut, (list.size() - cut) * sizeof(adsb_modes_rec)) == 0);
        }
    }
    { // nothing at all; argument errors
        const Result empty = run({}, {}, {});
        CHECK(empty.h.n == 0 && empty.h.n_known_out == 0);
        const Result only_known = run({}, all, {0, 0});
        CHECK(only_known.known == all);
        const uint32_t unsorted[2] = {5, 4}, twice[2] = {5, 5}, large[1] = {1u << 24};
        const uint64_t short_counts[1] = {199};
        CHECK(adsb_host_modes(list.data(), 200, nullptr, 0, unsorted, 2, nullptr, nullptr, nullptr, nullptr, nullptr) == ADSB_E_ARG);
        CHECK(adsb_host_modes(list.data(), 200, nullptr, 0, twice, 2, nullptr, nullptr, nullptr, nullptr, nullptr) == ADSB_E_ARG);
        CHECK(adsb_host_modes(list.data(), 200, nullptr, 0, large, 1, nullptr, nullptr, nullptr, nullptr, nullptr) == ADSB_E_ARG);
        CHECK(adsb_host_modes(nullptr, 200, nullptr, 0, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == ADSB_E_ARG);
        CHECK(adsb_host_modes(list.data(), 200, nullptr, 0, nullptr, 1, nullptr, nullptr, nullptr, nullptr, nullptr) == ADSB_E_ARG);
        CHECK(adsb_host_modes(list.data(), 200, short_counts, 1, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == ADSB_E_ARG);
        CHECK(adsb_host_modes(list.data(), 200, short_counts, 0, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == ADSB_E_ARG);
        CHECK(adsb_host_modes(list.data(), (size_t)1 << 32, nullptr, 0, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == ADSB_E_CAPACITY);
    }
    wire_short();
    if (fails) std::printf("%d check(s) FAILED\n", fails);
    else std::printf("all checks passed\n");
    return fails ? 1 : 0;
}
