// replies_edges.cpp -- stand-alone sanitizer run of the CPU mirror of the replies scan and the list merge
// (adsb_host_replies and adsb_host_merge_lists, air_rs_amd/csrc/host/adsb_replies.cpp, which compiles the text the
// device compiles: air_rs_amd/csrc/adsb_replies.h).  Exact-size heap buffers for the samples in and the frames out, so
// that a read or write beside them is a heap-buffer-overflow: three touching channels of seeded noise, i8 and CS16, at
// the lengths around every bound of the window rule (26, the short and the long frame's 128 and 240, one less and one
// more) and two longer ones; without a filter, with a filter and a capacity of three, and the list merged with itself.
// Host sources only, no device:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/host/replies_edges.cpp
//       air_rs_amd/csrc/host/adsb_replies.cpp -o /tmp/replies_edges && /tmp/replies_edges   (one command)
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "../../include/adsb_host.h"

static int fails = 0;
#define CHECK(x)                                                     \
    do {                                                             \
        if (!(x)) { std::printf("FAILED line %d: %s\n", __LINE__, #x); ++fails; } \
    } while (0)

int main()
{
    unsigned long long frames = 0, preambles = 0;
    for (int st = 0; st < 2; ++st)
        for (size_t n : {26u, 27u, 127u, 128u, 129u, 239u, 240u, 241u, 5000u, 70001u}) {
            const size_t bytes = n * (st ? 4 : 2) * 3;
            char *iq = (char *)std::malloc(bytes);
            unsigned s = 12345u + (unsigned)n;
            for (size_t k = 0; k < bytes; ++k) iq[k] = (char)((s = s * 1664525u + 1013904223u) >> 24);
            adsb_replies_cfg cfg{};
            adsb_replies_header h{}, h2{};
            size_t got = 0;
            uint64_t counts[3], merged_counts[3];
            CHECK(adsb_host_replies(st, &cfg, iq, 3, n, n, nullptr, 0, nullptr, 0, &got, counts, &h) == ADSB_OK && got == 0);
            adsb_frame *out = (adsb_frame *)std::malloc(sizeof(adsb_frame) * (h.n_out ? h.n_out : 1));
            CHECK(adsb_host_replies(st, &cfg, iq, 3, n, n, nullptr, 0, out, h.n_out, &got, counts, &h2) == ADSB_OK);
            CHECK(got == h.n_out && h2.n_out == h.n_out && counts[0] + counts[1] + counts[2] == h.n_out);
            CHECK(h.total_found == h.n_all_call + h.n_df18 + h.n_address_parity && h.flags == 0 && h.n_not_known == 0);
            for (size_t k = 0; k < got; ++k) CHECK(out[k].offset + 128 <= n && out[k].status == 0 && out[k].fixed_bit == 0xFF);
            adsb_frame *m = (adsb_frame *)std::malloc(sizeof(adsb_frame) * (2 * got + 1));
            uint32_t *src = (uint32_t *)std::malloc(4 * (2 * got + 1));
            CHECK(adsb_host_merge_lists(out, counts, out, counts, 3, m, src, merged_counts) == ADSB_OK);
            for (size_t k = 0; k + 1 < 2 * got; k += 2)   // a list merged with itself: every frame twice, list A's first
                CHECK(m[k].offset == m[k + 1].offset && src[k] == k / 2 && src[k + 1] == (k / 2 | ADSB_MERGE_FROM_B));
            const uint32_t known[2] = {5, 0xFFFFFF};
            cfg.flags = ADSB_REPLIES_AP_KNOWN;
            cfg.max_frames = 3;
            CHECK(adsb_host_replies(st, &cfg, iq, 3, n, n, known, 2, out, h.n_out, &got, counts, &h2) == ADSB_OK);
            CHECK(h2.n_out <= 3 && h2.n_preamble == h.n_preamble && h2.n_not_known + h2.n_address_parity == h.n_address_parity);
            frames += h.n_out, preambles += h.n_preamble;
            std::free(src), std::free(m), std::free(out), std::free(iq);
        }
    std::printf("replies_edges: %llu frames from %llu preambles, %d failures\n", frames, preambles, fails);
    return fails != 0;
}
