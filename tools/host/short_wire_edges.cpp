// short_wire_edges.cpp -- stand-alone sanitizer run of the CPU mirrors of the short-frame output
// (adsb_host_frame_levels_modes, air_rs_amd/csrc/host/adsb_levels.cpp over air_rs_amd/csrc/adsb_levels.h, and
// adsb_host_wire_encode with ADSB_WIRE_SHORT over air_rs_amd/csrc/adsb_wire.h: the text the device compiles too).
// Exact-size heap buffers: a sample read at or past w + 128 of a short frame at the end of the buffer, a frame byte read
// at or past a 7-byte frame's end, or an output byte past `cap` is a heap-buffer-overflow.  Host sources only, no device:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/host/short_wire_edges.cpp \
//       air_rs_amd/csrc/host/adsb_levels.cpp air_rs_amd/csrc/host/adsb_wire.cpp -o /tmp/short_wire_edges && /tmp/short_wire_edges
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

#include "../../include/adsb_host.h"

static int fails = 0;
#define CHECK(x)                                                     \
    do {                                                             \
        if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); ++fails; } \
    } while (0)

static adsb_frame frame_of(uint8_t first, uint64_t offset)
{
    adsb_frame f;
    std::memset(&f, 0, sizeof(f));
    f.offset = offset;
    for (int b = 0; b < 14; ++b) f.bytes[b] = (uint8_t)(0x1A + 37 * b);
    f.bytes[0] = first;
    return f;
}

template <typename T>
static void levels(int sample_type)
{
    for (size_t n : {127u, 128u, 129u, 240u, 241u, 367u}) {
        for (uint32_t channels : {1u, 3u}) {
            T *iq = static_cast<T *>(std::malloc(2 * sizeof(T) * n * channels)); // exactly the channels: nothing behind them
            for (size_t k = 0; k < 2 * n * channels; ++k) iq[k] = (T)(k % 7 == 0 ? -128 : (int)(k % 251) - 125);
            // per channel: short frames at 0, n-128, n-127 and long ones at 0, n-240, n-239 (negative ones wrap to huge offsets)
            const size_t per = 6, total = per * channels;
            adsb_frame *fr = static_cast<adsb_frame *>(std::malloc(sizeof(adsb_frame) * total));
            uint64_t *counts = static_cast<uint64_t *>(std::malloc(8 * channels));
            for (uint32_t c = 0; c < channels; ++c) {
                counts[c] = per;
                const uint64_t at[per] = {0, (uint64_t)n - 128, (uint64_t)n - 127, 0, (uint64_t)n - 240, (uint64_t)n - 239};
                for (size_t k = 0; k < per; ++k) fr[c * per + k] = frame_of(k < 3 ? 0x78 : 0x80, 1000 + at[k]); // DF15, DF16
            }
            adsb_frame_level *out = static_cast<adsb_frame_level *>(std::malloc(sizeof(adsb_frame_level) * total));
            CHECK(adsb_host_frame_levels_modes(sample_type, iq, channels, n, n, 1000, fr, counts, total, out) == ADSB_OK);
            for (uint32_t c = 0; c < channels; ++c) {
                const adsb_frame_level *r = out + c * per;
                CHECK(r[0].flags == (n >= 128 ? 3 : 0) && r[1].flags == (n >= 128 ? 3 : 0) && r[2].flags == 0);
                CHECK(r[3].flags == (n >= 240 ? 1 : 0) && r[4].flags == (n >= 240 ? 1 : 0) && r[5].flags == 0);
                CHECK(r[2].signal_sum == 0 && r[5].peak == 0);
            }
            std::free(out), std::free(counts), std::free(fr), std::free(iq);
        }
    }
}

static void wire()
{
    // seven-byte frames in an exact-size buffer: the encoder may not look at bytes[7..14) of the last one
    const size_t n = 5;
    uint8_t *raw = static_cast<uint8_t *>(std::malloc(sizeof(adsb_frame) * n - 7 - 2)); // the last frame ends behind bytes[6]
    for (size_t i = 0; i < n; ++i) {
        adsb_frame f = frame_of(i % 2 ? 0x1A : 0x20, 0x1A1A1A1A1A1Aull / 6 + i);
        std::memcpy(raw + sizeof(adsb_frame) * i, &f, i + 1 < n ? sizeof(adsb_frame) : sizeof(adsb_frame) - 9);
    }
    const adsb_frame *fr = reinterpret_cast<const adsb_frame *>(raw);
    adsb_frame_level lv[n];
    std::memset(lv, 0, sizeof(lv));
    for (size_t i = 0; i < n; ++i) lv[i].signal_sum = 60ull * 32768 * (i + 1) / 8, lv[i].flags = (uint16_t)(i % 3 ? 3 : 1);
    for (uint32_t format : {0x100u, 0x101u, 0x102u}) {
        adsb_wire_cfg cfg = {format, 1, 5};
        size_t total = 0;
        uint32_t ends[n];
        CHECK(adsb_host_wire_encode(&cfg, ADSB_SAMPLE_I8, fr, lv, n, nullptr, 0, &total, ends) == ADSB_OK);
        CHECK(total == ends[n - 1] && total >= 16 * n && total <= 30 * n);
        for (size_t cap = 0; cap <= total; ++cap) {
            uint8_t *out = static_cast<uint8_t *>(std::malloc(cap ? cap : 1));
            size_t nb = 0;
            CHECK(adsb_host_wire_encode(&cfg, ADSB_SAMPLE_I8, fr, lv, n, out, cap, &nb, nullptr) == ADSB_OK && nb == total);
            std::free(out);
        }
    }
    adsb_wire_cfg bad = {0x103u, 0, 0};
    size_t nb = 0;
    CHECK(adsb_host_wire_encode(&bad, ADSB_SAMPLE_I8, fr, nullptr, n, nullptr, 0, &nb, nullptr) == ADSB_E_ARG);
    std::free(raw);
}

int main()
{
    levels<int8_t>(ADSB_SAMPLE_I8);
    levels<int16_t>(ADSB_SAMPLE_I16);
    wire();
    std::printf(fails ? "short_wire_edges: %d checks failed\n" : "short_wire_edges: ok\n", fails);
    return fails ? 1 : 0;
}
