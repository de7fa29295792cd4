// levels_edges.cpp -- stand-alone sanitizer run of the CPU mirror of the per-frame levels (adsb_host_frame_levels,
// air_rs_amd/csrc/host/adsb_levels.cpp): the one piece of that feature that indexes caller memory on the CPU.  Exact-size
// heap buffers, windows on the first and on the last sample, and every kind of window that does not fit, so that a read
// one sample outside the buffer is a heap-buffer-overflow.  Host sources only, no device:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/host/levels_edges.cpp air_rs_amd/csrc/host/adsb_levels.cpp -o /tmp/levels_edges && /tmp/levels_edges
#include <cmath>
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

template <typename T>
static void run(int sample_type, size_t n_samples, uint64_t first)
{
    T *iq = static_cast<T *>(std::malloc(n_samples * 2 * sizeof(T) + (n_samples ? 0 : 1))); // exactly the buffer
    const T lo = sample_type == ADSB_SAMPLE_I8 ? (T)-128 : (T)-32768;
    for (size_t j = 0; j < n_samples; ++j) { // a full-scale sample every 50: several in every window
        iq[2 * j] = j % 50 == 0 ? lo : (T)(j % 5);
        iq[2 * j + 1] = j % 50 == 0 ? lo : (T)(j % 3);
    }
    const uint64_t offs[] = {first, first + 1, first + n_samples - 240, first + n_samples - 239, first + n_samples,
                             first - 1, 0, 239, ~0ull, 1ull << 63, first + (n_samples >= 240 ? (n_samples - 240) / 2 : 0)};
    const size_t n = sizeof(offs) / sizeof(offs[0]);
    adsb_frame *fr = static_cast<adsb_frame *>(std::malloc(n * sizeof(adsb_frame)));
    adsb_frame_level *out = static_cast<adsb_frame_level *>(std::malloc(n * sizeof(adsb_frame_level)));
    for (size_t i = 0; i < n; ++i) {
        std::memset(&fr[i], 0, sizeof(fr[i]));
        fr[i].offset = offs[i];
        for (int b = 0; b < 14; ++b) fr[i].bytes[b] = (uint8_t)(0x8D + 37 * b + 11 * i);
    }
    std::memset(out, 0xEE, n * sizeof(adsb_frame_level));
    CHECK(adsb_host_frame_levels(sample_type, iq, n_samples, first, fr, n, out) == ADSB_OK);
    size_t valid = 0;
    for (size_t i = 0; i < n; ++i) {
        const bool fits = n_samples >= 240 && offs[i] >= first && offs[i] - first <= n_samples - 240;
        CHECK(out[i].flags == (fits ? ADSB_LEVEL_VALID : 0));
        if (fits) {
            ++valid;
            CHECK(out[i].peak >= out[i].pulse_min && out[i].peak >= out[i].quiet_max && out[i].weak_bits <= 112);
            CHECK(out[i].peak == (sample_type == ADSB_SAMPLE_I8 ? 32768u : 2147483648u)); // (lo, lo) occurs in every window
        } else {
            static const adsb_frame_level zero = {};
            CHECK(std::memcmp(&out[i], &zero, sizeof(zero)) == 0);
        }
    }
    std::printf("sample_type %d, %zu samples from %llu: %zu of %zu frames valid\n", sample_type, n_samples,
                (unsigned long long)first, valid, n);
    std::free(out);
    std::free(fr);
    std::free(iq);
}

int main()
{
    const size_t sizes[] = {0, 1, 239, 240, 241, 1000};
    for (size_t n : sizes)
        for (uint64_t first : {0ull, 1ull, 5000ull, 1ull << 40}) {
            run<int8_t>(ADSB_SAMPLE_I8, n, first);
            run<int16_t>(ADSB_SAMPLE_I16, n, first);
        }
    CHECK(adsb_level_dbfs(ADSB_SAMPLE_I8, 116ull * 32768, 116) == 0.0);
    CHECK(adsb_level_dbfs(ADSB_SAMPLE_I16, 124ull << 31, 124) == 0.0);
    CHECK(std::isinf(adsb_level_dbfs(ADSB_SAMPLE_I8, 0, 116)) && adsb_level_dbfs(ADSB_SAMPLE_I8, 0, 116) < 0);
    CHECK(std::isnan(adsb_level_dbfs(7, 1, 1)) && std::isnan(adsb_level_dbfs(ADSB_SAMPLE_I8, 1, 0)));
    CHECK(adsb_host_frame_levels(ADSB_SAMPLE_I8, nullptr, 0, 0, nullptr, 0, nullptr) == ADSB_E_ARG);
    if (fails) std::printf("%d check(s) FAILED\n", fails);
    else std::printf("all checks passed\n");
    return fails ? 1 : 0;
}
