// adsb_commb.cpp -- CPU mirror of the device's Comm-B stage (adsb_commb.hip): adsb_host_commb and adsb_host_commb_as
// of include/adsb_host.h.  The record of one frame is ../adsb_commb.h, the text the device compiles; here the frames
// in sequence and the totals as they come.  No device.
#include "../../../include/adsb_host.h"
#include "../adsb_commb.h"

extern "C" int adsb_host_commb(const adsb_frame *frames, size_t n, adsb_commb_rec *recs, adsb_commb_header *header)
{
    using namespace adsbk;
    const int rc = commb_args_check(frames, n);
    if (rc != ADSB_OK) return rc;
    uint64_t total[kCommbTallies] = {};
    for (size_t j = 0; j < n; ++j) {
        const adsb_commb_rec r = commb_first(modes_bytes(frames[j].bytes));
        total[r.state] += 1;
        const uint32_t reg = commb_register_tally(r);
        if (reg < kCommbTallies) total[reg] += 1;
        if (recs) recs[j] = r;
    }
    if (header) commb_header_of(n, total, header);
    return ADSB_OK;
}

extern "C" int adsb_host_commb_as(const uint8_t bytes[14], uint32_t bds, adsb_commb_rec *rec)
{
    using namespace adsbk;
    if (!bytes || !rec) return ADSB_E_ARG;
    const ModesBytes b = modes_bytes(bytes);
    adsb_commb_rec r = commb_first(b);
    const uint32_t c = commb_bit_of(bds);
    if (c == 0u || (r.candidates & c) == 0u) return ADSB_E_ARG;
    commb_decode(commb_mb(b), c, r);
    *rec = r;
    return ADSB_OK;
}
