// wire_edges.cpp -- stand-alone sanitizer run of the CPU mirror of the wire output (adsb_host_wire_encode,
// air_rs_amd/csrc/host/adsb_wire.cpp over air_rs_amd/csrc/adsb_wire.h, the text the device compiles too): the piece of
// that feature that writes caller memory on the CPU.  Exact-size heap buffers, so that one byte written past `cap`, or
// one entry past ends[n], is a heap-buffer-overflow; `cap` one byte short of, at, and one past every frame boundary; the
// frame whose 21 payload bytes are all 0x1A; timestamps across 2^48 and 2^64; the signal byte at its extremes.  Host
// sources only, no device:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/host/wire_edges.cpp air_rs_amd/csrc/host/adsb_wire.cpp -o /tmp/wire_edges && /tmp/wire_edges
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

static std::vector<adsb_frame> frames_of(const std::vector<uint64_t> &offs, int pattern)
{
    std::vector<adsb_frame> fr(offs.size());
    for (size_t i = 0; i < fr.size(); ++i) {
        std::memset(&fr[i], 0, sizeof(fr[i]));
        fr[i].offset = offs[i];
        for (int b = 0; b < 14; ++b)
            fr[i].bytes[b] = pattern == 0 ? kKnown[b] : pattern == 1 ? (uint8_t)0x1A : (uint8_t)((i + b) % 3 ? 0x1A : 0x8D + 7 * b);
    }
    return fr;
}

// the whole stream into an exact-size buffer, then every cap around every boundary into exact-size buffers
static void run(uint32_t format, int sample_type, const std::vector<adsb_frame> &fr, const std::vector<adsb_frame_level> *lv,
                uint64_t bias)
{
    const size_t n = fr.size();
    adsb_wire_cfg cfg = {format, lv ? 1u : 0u, bias};
    size_t total = 0;
    CHECK(adsb_host_wire_encode(&cfg, sample_type, fr.data(), lv ? lv->data() : nullptr, n, nullptr, 0, &total, nullptr) == ADSB_OK);
    uint8_t *full = static_cast<uint8_t *>(std::malloc(total ? total : 1));
    uint32_t *ends = static_cast<uint32_t *>(std::malloc(n ? n * sizeof(uint32_t) : 1));
    size_t again = 0;
    CHECK(adsb_host_wire_encode(&cfg, sample_type, fr.data(), lv ? lv->data() : nullptr, n, full, total, &again, ends) == ADSB_OK);
    CHECK(again == total && (n == 0 || ends[n - 1] == total));
    size_t prev = 0;
    for (size_t i = 0; i < n; ++i) {
        const size_t len = ends[i] - prev;
        CHECK(format == ADSB_WIRE_BEAST ? (len >= 23 && len <= 44 && full[prev] == 0x1A && full[prev + 1] == 0x33)
              : format == ADSB_WIRE_AVR ? (len == 31 && full[prev] == '*' && full[ends[i] - 1] == '\n')
                                        : (len == 43 && full[prev] == '@' && full[ends[i] - 1] == '\n'));
        prev = ends[i];
    }
    size_t caps = 0;
    for (size_t i = 0; i <= n; ++i) {
        const size_t edge = i ? ends[i - 1] : 0;
        for (int d = -1; d <= 1; ++d) {
            if (edge == 0 && d < 0) continue;
            const size_t cap = edge + d;
            uint8_t *out = static_cast<uint8_t *>(std::malloc(cap ? cap : 1)); // exactly cap bytes
            uint32_t *e2 = static_cast<uint32_t *>(std::malloc(n ? n * sizeof(uint32_t) : 1));
            size_t nb = 0;
            CHECK(adsb_host_wire_encode(&cfg, sample_type, fr.data(), lv ? lv->data() : nullptr, n, out, cap, &nb, e2) == ADSB_OK);
            size_t want = 0; // whole frames only
            for (size_t k = 0; k < n; ++k)
                if (ends[k] <= cap) want = ends[k];
            CHECK(nb == total);
            CHECK(std::memcmp(out, full, want) == 0);
            CHECK(n == 0 || std::memcmp(e2, ends, n * sizeof(uint32_t)) == 0);
            std::free(e2);
            std::free(out);
            ++caps;
        }
    }
    std::printf("format %u, sample_type %d, %zu frames, bias %llu: %zu bytes, %zu caps\n", format, sample_type, n,
                (unsigned long long)bias, total, caps);
    std::free(ends);
    std::free(full);
}

int main()
{
    const uint64_t wrap = (1ull << 48) / 6, all1a = 0x1A1A1A1A1A1Aull / 6;
    const std::vector<uint64_t> offs = {0, 1, all1a, wrap - 1, wrap, wrap + 1, ~0ull, 1ull << 63, ~0ull / 6, ~0ull / 6 + 1, all1a};
    for (uint32_t format : {ADSB_WIRE_BEAST, ADSB_WIRE_AVR, ADSB_WIRE_AVR_MLAT})
        for (int pattern = 0; pattern < 3; ++pattern) {
            const std::vector<adsb_frame> fr = frames_of(offs, pattern);
            for (int st : {ADSB_SAMPLE_I8, ADSB_SAMPLE_I16}) {
                const uint64_t unit = 116ull * (st == ADSB_SAMPLE_I8 ? 32768ull : 2147483648ull);
                std::vector<adsb_frame_level> lv(fr.size());
                const uint64_t sums[] = {0, 1, unit, unit - 1, unit + 1, ~0ull, unit / 96, 12345, unit / 2, 1ull << 63, unit / 96 + 1};
                for (size_t i = 0; i < lv.size(); ++i) {
                    std::memset(&lv[i], 0, sizeof(lv[i]));
                    lv[i].signal_sum = sums[i % (sizeof(sums) / sizeof(sums[0]))];
                    lv[i].flags = i == 7 ? 0 : ADSB_LEVEL_VALID;
                }
                run(format, st, fr, nullptr, 0);
                run(format, st, fr, &lv, (1ull << 48) - 1);
            }
            run(format, ADSB_SAMPLE_I8, std::vector<adsb_frame>(), nullptr, 5);                       // n = 0
            run(format, ADSB_SAMPLE_I8, std::vector<adsb_frame>(fr.begin() + 2, fr.begin() + 3), nullptr, 0); // n = 1
        }
    { // the literal known answer, and the frame of 44 bytes
        adsb_wire_cfg cfg = {ADSB_WIRE_BEAST, 0, 0};
        const std::vector<adsb_frame> fr = frames_of({0}, 0);
        uint8_t out[23];
        size_t nb = 0;
        CHECK(adsb_host_wire_encode(&cfg, ADSB_SAMPLE_I8, fr.data(), nullptr, 1, out, sizeof(out), &nb, nullptr) == ADSB_OK);
        const uint8_t want[9] = {0x1A, 0x33, 0, 0, 0, 0, 0, 0, 0};
        CHECK(nb == 23 && std::memcmp(out, want, 9) == 0 && std::memcmp(out + 9, kKnown, 14) == 0);
        const std::vector<adsb_frame> hot = frames_of({all1a}, 1);
        adsb_frame_level lv;
        std::memset(&lv, 0, sizeof(lv));
        lv.flags = ADSB_LEVEL_VALID;
        for (lv.signal_sum = 1; lv.signal_sum < 116ull * 32768; ++lv.signal_sum) { // the first sum whose byte is 0x1A
            uint8_t o[44];
            cfg.signal = 1;
            CHECK(adsb_host_wire_encode(&cfg, ADSB_SAMPLE_I8, hot.data(), &lv, 1, o, sizeof(o), &nb, nullptr) == ADSB_OK);
            if (nb == 44) {
                for (int k = 2; k < 44; ++k) CHECK(o[k] == 0x1A);
                break;
            }
            lv.signal_sum += 97;
        }
        CHECK(nb == 44);
    }
    { // argument errors
        adsb_wire_cfg bad_format = {3, 0, 0}, bad_bias = {ADSB_WIRE_AVR, 0, 1ull << 48}, ok = {ADSB_WIRE_AVR, 0, 0};
        const std::vector<adsb_frame> fr = frames_of({0}, 0);
        size_t nb = 7;
        uint8_t out[31];
        CHECK(adsb_host_wire_encode(nullptr, ADSB_SAMPLE_I8, fr.data(), nullptr, 1, out, 31, &nb, nullptr) == ADSB_E_ARG);
        CHECK(adsb_host_wire_encode(&bad_format, ADSB_SAMPLE_I8, fr.data(), nullptr, 1, out, 31, &nb, nullptr) == ADSB_E_ARG);
        CHECK(adsb_host_wire_encode(&bad_bias, ADSB_SAMPLE_I8, fr.data(), nullptr, 1, out, 31, &nb, nullptr) == ADSB_E_ARG);
        CHECK(adsb_host_wire_encode(&ok, 2, fr.data(), nullptr, 1, out, 31, &nb, nullptr) == ADSB_E_ARG);
        CHECK(adsb_host_wire_encode(&ok, ADSB_SAMPLE_I8, nullptr, nullptr, 1, out, 31, &nb, nullptr) == ADSB_E_ARG);
        CHECK(adsb_host_wire_encode(&ok, ADSB_SAMPLE_I8, fr.data(), nullptr, 1, nullptr, 31, &nb, nullptr) == ADSB_E_ARG);
        CHECK(adsb_host_wire_encode(&ok, ADSB_SAMPLE_I8, fr.data(), nullptr, 1, out, 31, nullptr, nullptr) == ADSB_E_ARG);
        CHECK(nb == 7);
        CHECK(adsb_host_wire_encode(&ok, ADSB_SAMPLE_I8, fr.data(), nullptr, 1, out, 31, &nb, nullptr) == ADSB_OK && nb == 31);
    }
    if (fails) std::printf("%d check(s) FAILED\n", fails);
    else std::printf("all checks passed\n");
    return fails ? 1 : 0;
}
