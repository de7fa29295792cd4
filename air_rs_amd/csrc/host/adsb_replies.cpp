// adsb_replies.cpp -- CPU mirror of the device's replies scan and list merge (adsb_replies.hip): adsb_host_replies and
// adsb_host_merge_lists of include/adsb_host.h.  The text of one offset, of one frame and of a frame's place in a merge
// is ../adsb_replies.h, the text the device compiles; here the offsets in sequence and the totals as they come.  No
// device.
#include <string.h>

#include "../../../include/adsb_host.h"
#include "../adsb_replies.h"

namespace {

template <int ST>
struct HostPower {
    const void *iq; // the channel's sample 0
    uint32_t operator()(uint64_t k) const { return adsbk::replies_sample_power<ST>(iq, k); }
};

template <int ST>
void scan(const adsb_replies_cfg *cfg, const void *iq, uint32_t n_channels, size_t n_samples, size_t stride,
          const uint32_t *known, uint32_t n_known, uint64_t cap, adsb_frame *out, size_t max_out, uint64_t *counts,
          uint64_t *totals)
{
    using namespace adsbk;
    const size_t sample_bytes = ST == ADSB_SAMPLE_I8 ? 2 : 4;
    uint64_t kept = 0;
    for (uint32_t c = 0; c < n_channels; ++c) {
        const HostPower<ST> p{static_cast<const char *>(iq) + sample_bytes * stride * c};
        uint64_t in_list = 0;
        for (uint64_t i = 0; i + kRepliesDfSpan <= n_samples; ++i) {
            if (!replies_preamble(p, i)) continue;
            ModesBytes b{0, 0};
            const uint32_t o = replies_candidate(p, i, n_samples, cfg->flags, known, n_known, &b);
            totals[0] += 1;
            if (o >= kRepliesAllCall) totals[o - 1u] += 1;
            if (!replies_kept(o)) continue;
            if (kept < cap) {
                if (kept < max_out) {
                    const RepliesFrameWords w = replies_frame(cfg->first_sample_index + i, b);
                    memcpy(&out[kept], w.w, sizeof(adsb_frame));
                }
                in_list += 1;
            }
            kept += 1;
        }
        if (counts) counts[c] = in_list;
    }
}

} // namespace

extern "C" int adsb_host_replies(int sample_type, const adsb_replies_cfg *cfg, const void *iq, uint32_t n_channels,
                                 size_t n_samples, size_t channel_stride, const uint32_t *known, size_t n_known,
                                 adsb_frame *out, size_t max_out, size_t *n_out, uint64_t *counts, adsb_replies_header *header)
{
    using namespace adsbk;
    if ((sample_type != ADSB_SAMPLE_I8 && sample_type != ADSB_SAMPLE_I16) || (!out && max_out)) return ADSB_E_ARG;
    const int rc = replies_args_check(cfg, iq, n_channels, n_samples, channel_stride, known, n_known, true);
    if (rc != ADSB_OK) return rc;
    if (n_channels == 1) channel_stride = n_samples;
    const uint64_t cap = cfg->max_frames ? cfg->max_frames : ~0ull;
    uint64_t totals[kRepliesTallies] = {};
    if (sample_type == ADSB_SAMPLE_I8)
        scan<ADSB_SAMPLE_I8>(cfg, iq, n_channels, n_samples, channel_stride, known, (uint32_t)n_known, cap, out, max_out, counts, totals);
    else
        scan<ADSB_SAMPLE_I16>(cfg, iq, n_channels, n_samples, channel_stride, known, (uint32_t)n_known, cap, out, max_out, counts, totals);
    adsb_replies_header h;
    replies_header_of(totals, cap, &h);
    if (n_out) *n_out = (size_t)(h.n_out < max_out ? h.n_out : max_out);
    if (header) *header = h;
    return ADSB_OK;
}

extern "C" int adsb_host_merge_lists(const adsb_frame *a, const uint64_t *counts_a, const adsb_frame *b, const uint64_t *counts_b,
                                     uint32_t n_channels, adsb_frame *out, uint32_t *src, uint64_t *counts_out)
{
    using namespace adsbk;
    const int rc = merge_args_check(a, counts_a, b, counts_b, n_channels);
    if (rc != ADSB_OK) return rc;
    uint64_t *pa = new uint64_t[2 * ((size_t)n_channels + 1)], *pb = pa + n_channels + 1;
    pa[0] = pb[0] = 0;
    for (uint32_t c = 0; c < n_channels; ++c) pa[c + 1] = pa[c] + counts_a[c], pb[c + 1] = pb[c] + counts_b[c];
    const uint64_t na = pa[n_channels], nb = pb[n_channels];
    int ret = ADSB_OK;
    if (na >= ADSB_MERGE_FROM_B || nb >= ADSB_MERGE_FROM_B) ret = ADSB_E_CAPACITY;
    else if ((!a && na) || (!b && nb) || (!out && na + nb)) ret = ADSB_E_ARG;
    if (ret == ADSB_OK) {
        for (uint64_t k = 0; k < na; ++k) {
            const uint64_t at = replies_merge_place(a, pa, b, pb, n_channels, k, false);
            out[at] = a[k];
            if (src) src[at] = (uint32_t)k;
        }
        for (uint64_t k = 0; k < nb; ++k) {
            const uint64_t at = replies_merge_place(b, pb, a, pa, n_channels, k, true);
            out[at] = b[k];
            if (src) src[at] = (uint32_t)k | ADSB_MERGE_FROM_B;
        }
        if (counts_out)
            for (uint32_t c = 0; c < n_channels; ++c) counts_out[c] = counts_a[c] + counts_b[c];
    }
    delete[] pa;
    return ret;
}
