// adsb_modes.cpp -- CPU mirror of the device's Mode S stage (adsb_modes.hip): adsb_host_modes of include/adsb_host.h.
// The record of one frame and the known rule are ../adsb_modes.h, the text the device compiles; here the same plan in
// sequence: the records, one stable sort of (address, 1 + index) entries behind known_in's, the heads, the lookups.
// No device.
#include "../../../include/adsb_host.h"
#include "../adsb_modes.h"

#include <algorithm>
#include <utility>
#include <vector>

extern "C" int adsb_host_modes(const adsb_frame *frames, size_t n, const uint64_t *counts, uint32_t n_receivers,
                               const uint32_t *known_in, size_t n_known_in, adsb_modes_rec *recs, uint32_t *known_out,
                               adsb_frame *squitters, uint64_t *squitter_counts, adsb_modes_header *header)
{
    using namespace adsbk;
    const int rc = modes_args_check(frames, n, counts, n_receivers, known_in, n_known_in, true);
    if (rc != ADSB_OK) return rc;

    std::vector<adsb_modes_rec> rec(n);
    std::vector<std::pair<uint32_t, uint32_t>> entry; // (address, 0 for known_in or 1 + the list index)
    entry.reserve(n_known_in + n);
    for (size_t k = 0; k < n_known_in; ++k) entry.emplace_back(known_in[k], 0u);
    for (size_t j = 0; j < n; ++j) {
        rec[j] = modes_first(frames[j].bytes);
        if (modes_teaches(rec[j])) entry.emplace_back(rec[j].address, (uint32_t)j + 1u);
    }
    std::stable_sort(entry.begin(), entry.end(),
                     [](const std::pair<uint32_t, uint32_t> &a, const std::pair<uint32_t, uint32_t> &b) { return a.first < b.first; });
    std::vector<uint32_t> known, first; // the first entry of every run is the earliest
    for (size_t p = 0; p < entry.size(); ++p)
        if (p == 0 || entry[p].first != entry[p - 1].first) {
            known.push_back(entry[p].first);
            first.push_back(entry[p].second);
        }

    adsb_modes_header h{};
    h.n = n;
    h.n_known_out = known.size();
    uint64_t kinds[5] = {0, 0, 0, 0, 0};
    size_t j = 0;
    const uint32_t R = counts ? n_receivers : 1u;
    for (uint32_t r = 0; r < R; ++r) {
        const uint64_t before = h.n_squitters;
        const size_t end = counts ? j + (size_t)counts[r] : n;
        for (; j < end; ++j) {
            adsb_modes_rec &x = rec[j];
            if (x.kind == ADSB_MODES_UNKNOWN &&
                modes_is_known(known.data(), first.data(), (uint32_t)known.size(), x.address, (uint32_t)j))
                x.kind = ADSB_MODES_KNOWN;
            kinds[x.kind] += 1;
            if (modes_is_squitter(x)) {
                if (squitters) squitters[h.n_squitters] = frames[j];
                h.n_squitters += 1;
            }
            if (recs) recs[j] = x;
        }
        if (counts && squitter_counts) squitter_counts[r] = h.n_squitters - before;
    }
    h.n_self = kinds[ADSB_MODES_SELF];
    h.n_known = kinds[ADSB_MODES_KNOWN];
    h.n_unknown = kinds[ADSB_MODES_UNKNOWN];
    h.n_parity = kinds[ADSB_MODES_PARITY];
    h.n_unsupported = kinds[ADSB_MODES_UNSUPPORTED];
    if (known_out) std::copy(known.begin(), known.end(), known_out);
    if (header) *header = h;
    return ADSB_OK;
}
