// wire_in_edges.cpp -- stand-alone sanitizer run of the CPU mirror of the wire input (adsb_host_wire_parse,
// air_rs_amd/csrc/host/adsb_wire_in.cpp over air_rs_amd/csrc/adsb_wire_in.h, the text the device compiles too): the
// piece of that feature that reads and writes caller memory on the CPU.  Exact-size heap buffers, so that one byte read
// past a stream's end, or one record written past `max`, is a heap-buffer-overflow: every stream cut at every length
// (a reader that looks for the partner of a final 0x1A, or for the ';' behind the last digit, would read one past);
// every `max` from 0 to one past the frames that exist; the densest hostile streams; runs of 0x1A up to the end; several
// streams with empty ones among them; chunked parsing with the tail carried by `consumed`.  Host sources only, no device:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/host/wire_in_edges.cpp \
//       air_rs_amd/csrc/host/adsb_wire_in.cpp air_rs_amd/csrc/host/adsb_wire.cpp -o /tmp/wire_in_edges && /tmp/wire_in_edges
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

static const uint8_t kKnown[14] = {0x8D, 0x48, 0x40, 0xD6, 0x20, 0x2C, 0xC3, 0x71, 0xC3, 0x2C, 0xE0, 0x57, 0x60, 0x98};

struct Result {
    std::vector<adsb_frame> frames;
    std::vector<uint64_t> counts, consumed;
    adsb_wire_in_header h;
};

// One parse with every buffer at its exact size: the input (n bytes), `max` records of each kind, R counts and tails.
static Result parse(const adsb_wire_in_cfg &cfg, const std::vector<uint8_t> &in, const std::vector<uint64_t> &ends, size_t max)
{
    const size_t n = in.size(), R = ends.size();
    uint8_t *bytes = static_cast<uint8_t *>(std::malloc(n ? n : 1));
    if (n) std::memcpy(bytes, in.data(), n);
    uint64_t *e = static_cast<uint64_t *>(std::malloc(R * sizeof(uint64_t)));
    std::memcpy(e, ends.data(), R * sizeof(uint64_t));
    adsb_frame *fr = static_cast<adsb_frame *>(std::malloc(max ? max * sizeof(adsb_frame) : 1));
    adsb_wire_rx *rx = static_cast<adsb_wire_rx *>(std::malloc(max ? max * sizeof(adsb_wire_rx) : 1));
    adsb_frame_level *lv = static_cast<adsb_frame_level *>(std::malloc(max ? max * sizeof(adsb_frame_level) : 1));
    uint64_t *counts = static_cast<uint64_t *>(std::malloc(R * sizeof(uint64_t)));
    uint64_t *consumed = static_cast<uint64_t *>(std::malloc(R * sizeof(uint64_t)));
    Result r;
    size_t got = ~(size_t)0;
    CHECK(adsb_host_wire_parse(&cfg, n ? bytes : nullptr, n, e, (uint32_t)R, fr, rx, lv, max, &got, counts, consumed, &r.h) ==
          ADSB_OK);
    CHECK(got == (r.h.n_frames < max ? r.h.n_frames : max) && r.h.n_frames <= r.h.total_found);
    uint64_t sum = 0;
    for (size_t k = 0; k < R; ++k) {
        sum += counts[k];
        CHECK(consumed[k] <= ends[k] - (k ? ends[k - 1] : 0));
    }
    CHECK(sum == r.h.n_frames);
    for (size_t i = 0; i < got; ++i) {
        CHECK(fr[i].status == 0 && fr[i].fixed_bit == 0xFF && rx[i].receiver < R);
        CHECK((rx[i].kind == '3') == (cfg.format == ADSB_WIRE_BEAST));
        CHECK(!cfg.levels || (lv[i].flags == ADSB_LEVEL_VALID) == (rx[i].signal != 0));
    }
    r.frames.assign(fr, fr + got);
    r.counts.assign(counts, counts + R);
    r.consumed.assign(consumed, consumed + R);
    std::free(consumed), std::free(counts), std::free(lv), std::free(rx), std::free(fr), std::free(e), std::free(bytes);
    return r;
}

static std::vector<uint8_t> encoded(uint32_t format, size_t n, int pattern, uint64_t bias)
{
    std::vector<adsb_frame> fr(n);
    std::vector<adsb_frame_level> lv(n);
    for (size_t i = 0; i < n; ++i) {
        std::memset(&fr[i], 0, sizeof(fr[i]));
        std::memset(&lv[i], 0, sizeof(lv[i]));
        fr[i].offset = pattern == 1 ? 0x1A1A1A1A1A1Aull / 6 : 1000 * i + 7;
        for (int b = 0; b < 14; ++b)
            fr[i].bytes[b] = pattern == 0 ? kKnown[b] : pattern == 1 ? (uint8_t)0x1A : (uint8_t)((i + b) % 3 ? 0x1A : 0x8D + 7 * b);
        lv[i].signal_sum = pattern == 1 ? 38411 : 5000 * i; // 38411: the first i8 sum whose signal byte is 0x1A
        lv[i].flags = ADSB_LEVEL_VALID;
    }
    adsb_wire_cfg cfg = {format, 1, bias};
    std::vector<uint8_t> out(44 * n + 1);
    size_t total = 0;
    CHECK(adsb_host_wire_encode(&cfg, ADSB_SAMPLE_I8, fr.data(), lv.data(), n, out.data(), out.size(), &total, nullptr) == ADSB_OK);
    out.resize(total);
    return out;
}

static bool same_frames(const std::vector<adsb_frame> &a, const std::vector<adsb_frame> &b, size_t n)
{
    return n == 0 || (n <= a.size() && n <= b.size() && std::memcmp(a.data(), b.data(), n * sizeof(adsb_frame)) == 0);
}

// every prefix of the stream, then the stream in chunks with the tail carried: the same frames as the whole parse
static void cut_everywhere(const adsb_wire_in_cfg &cfg, const std::vector<uint8_t> &s, const char *what)
{
    const Result whole = parse(cfg, s, {s.size()}, s.size() / 23);
    size_t longest = 0;
    for (size_t c = 0; c <= s.size(); ++c) {
        const std::vector<uint8_t> head(s.begin(), s.begin() + c);
        const Result r = parse(cfg, head, {c}, c / 23);
        CHECK(r.h.n_frames <= whole.h.n_frames && c - r.consumed[0] <= 43);
        CHECK(same_frames(r.frames, whole.frames, r.frames.size()));
        longest = c - r.consumed[0] > longest ? c - r.consumed[0] : longest;
    }
    for (size_t chunk : {1, 2, 3, 7, 44, 45, 1000}) {
        std::vector<uint8_t> piece;
        std::vector<adsb_frame> all;
        for (size_t fed = 0; fed < s.size(); fed += chunk) {
            piece.insert(piece.end(), s.begin() + fed, s.begin() + (fed + chunk < s.size() ? fed + chunk : s.size()));
            const Result r = parse(cfg, piece, {piece.size()}, piece.size() / 23);
            all.insert(all.end(), r.frames.begin(), r.frames.end());
            piece.erase(piece.begin(), piece.begin() + r.consumed[0]);
            CHECK(piece.size() <= 43);
        }
        CHECK(all.size() == whole.frames.size() && same_frames(all, whole.frames, all.size()));
    }
    for (size_t max = 0; max <= whole.h.total_found + 1; ++max) { // output room from none to one more than needed
        const Result r = parse(cfg, s, {s.size()}, max);
        CHECK(r.frames.size() == (max < whole.h.n_frames ? max : whole.h.n_frames) && r.h.total_found == whole.h.total_found);
    }
    std::printf("%s: %zu bytes, %llu frames of %llu marks, longest tail %zu\n", what, s.size(),
                (unsigned long long)whole.h.n_frames, (unsigned long long)whole.h.n_marks, longest);
}

int main()
{
    const uint64_t top = (1ull << 48) - 1;
    for (uint32_t levels = 0; levels < 2; ++levels)
        for (int pattern = 0; pattern < 3; ++pattern) {
            adsb_wire_in_cfg beast = {ADSB_WIRE_BEAST, levels ? ADSB_WIRE_IN_CRC : 0u, levels ? top : 0, 0, ADSB_SAMPLE_I16, levels};
            cut_everywhere(beast, encoded(ADSB_WIRE_BEAST, 9, pattern, levels ? top : 0), "beast");
            adsb_wire_in_cfg avr = {ADSB_WIRE_AVR, levels ? ADSB_WIRE_IN_DF17 : 0u, 5, 0, ADSB_SAMPLE_I8, levels};
            cut_everywhere(avr, encoded(ADSB_WIRE_AVR, 9, pattern, 0), "avr *");
            avr.format = ADSB_WIRE_AVR_MLAT;
            cut_everywhere(avr, encoded(ADSB_WIRE_AVR_MLAT, 9, pattern, 5), "avr @");
        }
    { // hostile density and runs that reach the end, cut everywhere
        adsb_wire_in_cfg beast = {ADSB_WIRE_BEAST, 0, 0, 0, ADSB_SAMPLE_I8, 1}, avr = {ADSB_WIRE_AVR, 0, 0, 0, ADSB_SAMPLE_I8, 0};
        std::vector<uint8_t> dense, run(130, 0x1A), stars, digits(1, '@');
        for (int i = 0; i < 100; ++i) dense.push_back(0x1A), dense.push_back(0x33);
        cut_everywhere(beast, dense, "1A 33 x 100");
        cut_everywhere(beast, run, "1A x 130");
        run.insert(run.begin() + 77, 0x33);
        cut_everywhere(beast, run, "1A x 77, 33, 1A x 53");
        for (int i = 0; i < 120; ++i) stars.push_back(i % 7 == 3 ? '@' : '*');
        cut_everywhere(avr, stars, "* and @ x 120");
        for (int i = 0; i < 90; ++i) digits.push_back("0123456789abcdefABCDEF"[i % 22]);
        cut_everywhere(avr, digits, "@ and 90 digits");
        digits[41] = ';';
        cut_everywhere(avr, digits, "@, 40 digits, ;");
    }
    { // several streams, empty ones among them; a boundary that would make a frame of two streams' bytes
        std::vector<uint8_t> a = encoded(ADSB_WIRE_BEAST, 3, 2, 0), all = a;
        all.push_back(0x00), all.push_back(0x1A);                       // stream 0 ends in 1A ...
        const uint64_t e0 = all.size();
        all.insert(all.end(), a.begin() + 1, a.end());                  // ... stream 2 begins with 33 ...
        const uint64_t e2 = all.size();
        all.push_back(0x1A);
        adsb_wire_in_cfg cfg = {ADSB_WIRE_BEAST, 0, 0, 0, ADSB_SAMPLE_I8, 1};
        const Result r = parse(cfg, all, {e0, e0, e2, e2, all.size(), all.size()}, all.size() / 23);
        CHECK(r.counts == (std::vector<uint64_t>{3, 0, 2, 0, 0, 0}) && r.h.n_marks == 5);
        CHECK(r.consumed == (std::vector<uint64_t>{e0 - 1, 0, e2 - e0, 0, 0, 0}));
        cfg.max_frames = 4;
        const Result t = parse(cfg, all, {e0, e0, e2, e2, all.size(), all.size()}, 2);
        CHECK(t.counts == (std::vector<uint64_t>{3, 0, 1, 0, 0, 0}) && t.h.flags == ADSB_FLAG_TRUNCATED && t.frames.size() == 2);
        const Result none = parse(cfg, {}, {0, 0}, 0);
        CHECK(none.h.n_marks == 0 && none.consumed == (std::vector<uint64_t>{0, 0}));
    }
    { // argument errors; optional outputs left out
        adsb_wire_in_cfg ok = {ADSB_WIRE_BEAST, 0, 0, 0, 0, 0}, bad_format = {3, 0, 0, 0, 0, 0}, bad_bias = {0, 0, 1ull << 48, 0, 0, 0};
        adsb_wire_in_cfg bad_type = {0, 0, 0, 0, 2, 1};
        const std::vector<uint8_t> s = encoded(ADSB_WIRE_BEAST, 1, 0, 0);
        uint64_t end = s.size(), two[2] = {10, 5}, big = 1ull << 32;
        CHECK(adsb_host_wire_parse(&ok, s.data(), s.size(), &end, 1, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr) == ADSB_OK);
        CHECK(adsb_host_wire_parse(nullptr, s.data(), s.size(), &end, 1, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr) == ADSB_E_ARG);
        CHECK(adsb_host_wire_parse(&bad_format, s.data(), s.size(), &end, 1, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr) == ADSB_E_ARG);
        CHECK(adsb_host_wire_parse(&bad_bias, s.data(), s.size(), &end, 1, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr) == ADSB_E_ARG);
        CHECK(adsb_host_wire_parse(&bad_type, s.data(), s.size(), &end, 1, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr) == ADSB_E_ARG);
        CHECK(adsb_host_wire_parse(&ok, nullptr, s.size(), &end, 1, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr) == ADSB_E_ARG);
        CHECK(adsb_host_wire_parse(&ok, s.data(), s.size(), nullptr, 1, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr) == ADSB_E_ARG);
        CHECK(adsb_host_wire_parse(&ok, s.data(), s.size(), &end, 0, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr) == ADSB_E_ARG);
        CHECK(adsb_host_wire_parse(&ok, s.data(), s.size(), &end, 257, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr) == ADSB_E_ARG);
        CHECK(adsb_host_wire_parse(&ok, s.data(), s.size(), two, 2, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr) == ADSB_E_ARG);
        CHECK(adsb_host_wire_parse(&ok, s.data(), (size_t)big, &big, 1, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr) == ADSB_E_CAPACITY);
    }
    if (fails) std::printf("%d check(s) FAILED\n", fails);
    else std::printf("all checks passed\n");
    return fails ? 1 : 0;
}
