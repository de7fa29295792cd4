// correlate_edges.cpp -- stand-alone sanitizer run of the CPU mirror of correlate (adsb_host_correlate,
// air_rs_amd/csrc/host/adsb_correlate.cpp over air_rs_amd/csrc/adsb_correlate.h, the text the device compiles too): the
// piece of that feature that writes caller memory on the CPU.  Exact-size heap buffers, so that one message past
// max_msgs, or one reception past recs[n], is a heap-buffer-overflow; max_msgs of 0, one short of and at the message
// count; the chain boundary (gaps of window and window + 1, window 0 and 2^32 - 1); keys that differ in the last bit, the
// first bit and across the 64 / 48 bit split; times above 2^32 and 2^63; 256 receivers; receivers without frames; one
// group of a few thousand receptions.  Every result is checked against the invariants of the definition (and the
// group counts that the lists are built for).  Host sources only, no device:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       tools/host/correlate_edges.cpp air_rs_amd/csrc/host/adsb_correlate.cpp -o /tmp/correlate_edges && /tmp/correlate_edges
#include <algorithm>
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

struct Row {
    uint64_t offset;
    uint8_t bytes[14];
    uint8_t status, fixed_bit;
    uint64_t signal;
    uint16_t flags;
};

static Row row(uint64_t offset, const uint8_t *bytes = kKnown, uint8_t status = 0, uint8_t fixed = 0xFF, uint64_t signal = 0,
               uint16_t flags = 0)
{
    Row r;
    r.offset = offset;
    std::memcpy(r.bytes, bytes, 14);
    r.status = status;
    r.fixed_bit = fixed;
    r.signal = signal;
    r.flags = flags;
    return r;
}

// One list: per receiver its rows (sorted here by offset), the window, the bases; expect_msgs < 0: not checked.
static void run(const char *name, std::vector<std::vector<Row>> per, uint32_t window, const std::vector<uint64_t> *base,
                bool with_levels, long expect_msgs)
{
    const uint32_t R = (uint32_t)per.size();
    std::vector<uint64_t> counts(R);
    size_t n = 0;
    for (uint32_t r = 0; r < R; ++r) {
        std::stable_sort(per[r].begin(), per[r].end(), [](const Row &a, const Row &b) { return a.offset < b.offset; });
        counts[r] = per[r].size();
        n += per[r].size();
    }
    // exact-size heap copies of everything the mirror reads or writes
    adsb_frame *fr = static_cast<adsb_frame *>(std::malloc(n ? n * sizeof(adsb_frame) : 1));
    adsb_frame_level *lv = static_cast<adsb_frame_level *>(std::malloc(n ? n * sizeof(adsb_frame_level) : 1));
    std::vector<uint32_t> rx(n);
    size_t j = 0;
    for (uint32_t r = 0; r < R; ++r)
        for (const Row &x : per[r]) {
            std::memset(&fr[j], 0, sizeof(fr[j]));
            std::memset(&lv[j], 0, sizeof(lv[j]));
            fr[j].offset = x.offset;
            std::memcpy(fr[j].bytes, x.bytes, 14);
            fr[j].status = x.status;
            fr[j].fixed_bit = x.fixed_bit;
            lv[j].signal_sum = x.signal;
            lv[j].flags = x.flags;
            rx[j++] = r;
        }
    adsb_correlate_cfg cfg = {window, 0, 0};
    adsb_reception *recs = static_cast<adsb_reception *>(std::malloc(n ? n * sizeof(adsb_reception) : 1));
    size_t n_msgs = 0;
    const adsb_frame_level *levels = with_levels ? lv : nullptr;
    const uint64_t *b = base ? base->data() : nullptr;
    // the count alone: no room for messages
    CHECK(adsb_host_correlate(&cfg, n ? fr : nullptr, levels, n, counts.data(), R, b, nullptr, 0, &n_msgs, nullptr,
                              n ? recs : nullptr) == ADSB_OK);
    if (expect_msgs >= 0) CHECK(n_msgs == (size_t)expect_msgs);
    const size_t total = n_msgs;
    for (size_t room : {total, total ? total - 1 : 0, (size_t)0}) {
        adsb_message *msgs = static_cast<adsb_message *>(std::malloc(room ? room * sizeof(adsb_message) : 1));
        adsb_frame *fout = static_cast<adsb_frame *>(std::malloc(room ? room * sizeof(adsb_frame) : 1));
        size_t again = 0;
        CHECK(adsb_host_correlate(&cfg, n ? fr : nullptr, levels, n, counts.data(), R, b, msgs, room, &again, fout,
                                  n ? recs : nullptr) == ADSB_OK);
        CHECK(again == total);
        // the invariants of the definition, on what fits
        std::vector<char> seen(n, 0);
        size_t at = 0;
        for (size_t m = 0; m < std::min(room, total); ++m) {
            const adsb_message &g = msgs[m];
            CHECK(g.first == at && g.n_receptions >= 1 && at + g.n_receptions <= n);
            CHECK(std::memcmp(&g, &fout[m], sizeof(adsb_frame)) == 0 && fout[m].offset == g.time);
            CHECK(g.reserved == 0 && g.reserved2 == 0);
            if (m) {
                const int c = std::memcmp(msgs[m - 1].bytes, g.bytes, 14);
                CHECK(msgs[m - 1].time < g.time || (msgs[m - 1].time == g.time && c < 0));
            }
            std::vector<char> heard(256, 0);
            uint32_t n_rx = 0, n_clean = 0;
            uint8_t least = 0xFF;
            for (uint32_t k = 0; k < g.n_receptions; ++k) {
                const adsb_reception &x = recs[at + k];
                CHECK(x.frame < n && !seen[x.frame] && x.reserved == 0);
                if (x.frame >= n) continue;
                seen[x.frame] = 1;
                CHECK(x.receiver == rx[x.frame] && x.time == (b ? b[x.receiver] : 0) + fr[x.frame].offset);
                CHECK(std::memcmp(fr[x.frame].bytes, g.bytes, 14) == 0);
                if (k) {
                    const adsb_reception &p = recs[at + k - 1];
                    CHECK(p.time < x.time || (p.time == x.time && p.frame < x.frame));
                    CHECK(x.time - p.time <= window);
                }
                n_rx += heard[x.receiver] ? 0 : 1;
                heard[x.receiver] = 1;
                n_clean += fr[x.frame].status == 0;
                least = std::min(least, fr[x.frame].status);
            }
            CHECK(g.n_receivers == n_rx && g.n_clean == n_clean && g.status == least);
            CHECK(g.time == recs[at].time && g.span == recs[at + g.n_receptions - 1].time - g.time);
            CHECK(g.first_receiver == recs[at].receiver);
            if (!with_levels) CHECK(g.best_receiver == 0xFFFF && g.best_signal_sum == 0);
            at += g.n_receptions;
        }
        if (room >= total) CHECK(at == n);
        std::free(msgs);
        std::free(fout);
    }
    std::printf("%-28s n %6zu  receivers %3u  window %10u  messages %6zu\n", name, n, R, window, total);
    std::free(fr);
    std::free(lv);
    std::free(recs);
}

int main()
{
    // the chain boundary
    for (uint32_t w : {7u, 0u, 0xFFFFFFFFu}) {
        std::vector<std::vector<Row>> per(2);
        uint64_t t = 1000;
        const uint64_t gaps[7] = {w, w, (uint64_t)w + 1, w, (uint64_t)w + 1, (uint64_t)w + 1, w};
        for (int k = 0; k < 8; ++k) {
            per[k & 1].push_back(row(t));
            if (k < 7) t += gaps[k];
        }
        run("chain gaps", per, w, nullptr, false, 4);
    }
    {
        std::vector<std::vector<Row>> per(3);
        for (int k = 0; k < 3000; ++k) per[k % 3].push_back(row(100 + 5 * (uint64_t)k, kKnown, k % 7 == 0, (uint8_t)(k % 88),
                                                                (uint64_t)(k * 7919 % 1000), (uint16_t)(k % 4 != 0)));
        run("one long chain", per, 5, nullptr, true, 1);
        run("the same, window 4", per, 4, nullptr, true, 3000);
    }
    // key width
    {
        uint8_t base[14];
        std::memset(base, 0x40, 14);
        std::vector<std::vector<uint8_t>> keys;
        const int flips[][2] = {{-1, 0}, {13, 0}, {0, 7}, {5, 0}, {6, 7}, {6, 0}};
        for (const auto &f : flips) {
            std::vector<uint8_t> k(base, base + 14);
            if (f[0] >= 0) k[f[0]] ^= (uint8_t)(1u << f[1]);
            keys.push_back(k);
        }
        keys.push_back(std::vector<uint8_t>(14, 0x7F));
        keys.push_back(std::vector<uint8_t>(14, 0x80));
        keys.push_back(std::vector<uint8_t>(14, 0x00));
        keys.push_back(std::vector<uint8_t>(14, 0xFF));
        std::vector<std::vector<Row>> per(3);
        for (int r = 0; r < 3; ++r)
            for (size_t k = 0; k < keys.size(); ++k) per[r].push_back(row(500, keys[(k * 7 + r) % keys.size()].data()));
        run("key width", per, 0, nullptr, false, (long)keys.size());
    }
    // time width
    {
        const std::vector<uint64_t> base = {1ull << 33, (1ull << 63) + 5, 0, (1ull << 33) - 40};
        std::vector<std::vector<Row>> per(4);
        per[0] = {row(10), row(3000)};
        per[1] = {row(7), row(20)};
        per[2] = {row((1ull << 33) + 10), row((1ull << 63) + 12)};
        per[3] = {row(50), row(3040)};
        run("time width", per, 0, &base, false, 4);
    }
    // receivers
    {
        std::vector<std::vector<Row>> per(256);
        for (int r = 0; r < 256; ++r) per[r].push_back(row(1000 + (r * 37) % 50, kKnown, 0, 0xFF, (uint64_t)r, 1));
        run("256 receivers", per, 50, nullptr, true, 1);
        std::vector<std::vector<Row>> holes(9);
        holes[2] = {row(5), row(90)};
        holes[5] = {row(6), row(91)};
        holes[6] = {row(7)};
        run("receivers without frames", holes, 3, nullptr, false, 2);
        std::vector<std::vector<Row>> none(4);
        run("no frames", none, 3, nullptr, true, 0);
        std::vector<std::vector<Row>> twice(2);
        twice[0] = {row(10), row(12), row(500)};
        twice[1] = {row(11)};
        run("one receiver twice", twice, 2, nullptr, false, 2);
    }
    // rejected calls write nothing
    {
        adsb_correlate_cfg cfg = {1, 0, 0};
        adsb_frame f;
        std::memset(&f, 0, sizeof(f));
        adsb_reception rec;
        const uint64_t one = 1, two = 2;
        size_t n_msgs = 77;
        CHECK(adsb_host_correlate(&cfg, &f, nullptr, 1, &two, 1, nullptr, nullptr, 0, &n_msgs, nullptr, &rec) == ADSB_E_ARG);
        CHECK(adsb_host_correlate(&cfg, &f, nullptr, 1, &one, 0, nullptr, nullptr, 0, &n_msgs, nullptr, &rec) == ADSB_E_ARG);
        CHECK(adsb_host_correlate(nullptr, &f, nullptr, 1, &one, 1, nullptr, nullptr, 0, &n_msgs, nullptr, &rec) == ADSB_E_ARG);
        CHECK(n_msgs == 77);
    }
    std::printf(fails ? "correlate_edges: %d check(s) FAILED\n" : "correlate_edges: all checks passed\n", fails);
    return fails ? 1 : 0;
}
