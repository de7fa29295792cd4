// adsb_wire_in.cpp -- CPU mirror of the device's wire input (adsb_wire_in.hip): adsb_host_wire_parse of
// include/adsb_host.h.  The reader of one mark, the filters and the records are ../adsb_wire_in.h, the text the device
// compiles; here only the walk over each stream, one byte after the other.  No device.
#include "../../../include/adsb_host.h"
#include "../adsb_wire_in.h"

extern "C" int adsb_host_wire_parse(const adsb_wire_in_cfg *cfg, const uint8_t *bytes, size_t n_bytes,
                                    const uint64_t *stream_ends, uint32_t n_streams, adsb_frame *frames, adsb_wire_rx *rx,
                                    adsb_frame_level *levels, size_t max, size_t *n, uint64_t *counts, uint64_t *consumed,
                                    adsb_wire_in_header *header)
{
    if (!adsbk::wire_in_cfg_ok(cfg) || !stream_ends || (!bytes && n_bytes) || n_streams < 1 ||
        n_streams > adsbk::kWireInMaxStreams)
        return ADSB_E_ARG;
    if ((uint64_t)n_bytes > 0xFFFFFFFFull) return ADSB_E_CAPACITY;
    uint64_t prev = 0;
    for (uint32_t r = 0; r < n_streams; ++r) {
        if (stream_ends[r] < prev || stream_ends[r] > (uint64_t)n_bytes) return ADSB_E_ARG;
        prev = stream_ends[r];
    }
    if (prev != (uint64_t)n_bytes) return ADSB_E_ARG;
    const uint64_t most = adsbk::wire_in_most(cfg->filter, n_bytes);
    const uint64_t cap = cfg->max_frames ? (cfg->max_frames < most ? cfg->max_frames : most) : most;
    const bool beast = cfg->format == ADSB_WIRE_BEAST;
    adsbk::WireInTally tally{};
    uint64_t marks = 0, kept = 0; // (tally's own words are 32 bits wide: a span's on the device)
    uint64_t start = 0;
    for (uint32_t r = 0; r < n_streams; ++r) {
        const uint8_t *b = bytes + start;
        const uint32_t N = (uint32_t)(stream_ends[r] - start);
        const uint64_t kept_before = kept < cap ? kept : cap;
        uint32_t run = 0;         // 0x1A bytes in a row up to here
        uint64_t done = N;        // consumed, unless a mark is incomplete
        bool incomplete = false;
        for (uint32_t g = 0; g < N; ++g) {
            bool mark;
            if (beast) {
                run = b[g] == 0x1Au ? run + 1u : 0u;
                mark = (run & 1u) && g + 1u < N && b[g + 1u] != 0x1Au;
            } else {
                mark = b[g] == '*' || b[g] == '@';
            }
            if (!mark) continue;
            const adsbk::WireInMark m = adsbk::wire_in_read(beast, b, g, N);
            adsbk::WireInTally one{};
            const bool keep = adsbk::wire_in_count(m, cfg->filter, &one);
            marks += 1, tally.cut += one.cut, tally.unknown += one.unknown, tally.other += one.other;
            tally.rejected += one.rejected;
            if (m.state == adsbk::kWinIncomplete) {
                incomplete = true;
                done = g;
            }
            if (!keep) continue;
            if (kept < cap && kept < max) {
                if (frames) frames[kept] = adsbk::wire_in_frame(m, cfg->tick_bias);
                if (rx) rx[kept] = adsbk::wire_in_rx(m, g, r);
                if (levels && cfg->levels) levels[kept] = adsbk::wire_in_level(m.signal, cfg->sample_type);
            }
            ++kept;
        }
        if (beast && !incomplete) done = adsbk::wire_in_tail(N, run); // (run: the 0x1A bytes the stream ends with)
        if (counts) counts[r] = (kept < cap ? kept : cap) - kept_before;
        if (consumed) consumed[r] = done;
        start = stream_ends[r];
    }
    const uint64_t listed = kept < cap ? kept : cap;
    if (n) *n = (size_t)(listed < max ? listed : max);
    if (header) {
        adsb_wire_in_header h{};
        h.n_frames = listed;
        h.total_found = kept;
        h.n_marks = marks;
        h.n_cut = tally.cut;
        h.n_unknown = tally.unknown;
        h.n_other = tally.other;
        h.n_rejected = tally.rejected;
        h.flags = kept > cap ? ADSB_FLAG_TRUNCATED : 0u;
        *header = h;
    }
    return ADSB_OK;
}
