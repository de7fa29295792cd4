// adsb_es.cpp -- CPU mirror of the device's extended squitter status stage (adsb_es.hip): adsb_host_es and
// adsb_host_es_integrity of include/adsb_host.h.  The record of one frame and the integrity table are ../adsb_es.h, the
// text the device compiles; here the frames in sequence and the totals as they come.  No device.
#include "../../../include/adsb_host.h"
#include "../adsb_es.h"

extern "C" int adsb_host_es(const adsb_frame *frames, size_t n, adsb_es_rec *recs, adsb_es_header *header)
{
    using namespace adsbk;
    const int rc = es_args_check(frames, n);
    if (rc != ADSB_OK) return rc;
    uint64_t total[kEsTallies] = {};
    for (size_t j = 0; j < n; ++j) {
        const adsb_es_rec r = es_first(modes_bytes(frames[j].bytes));
        total[r.state] += 1;
        const uint32_t ver = es_version_tally(r);
        if (ver < kEsTallies) total[ver] += 1;
        if (recs) recs[j] = r;
    }
    if (header) es_header_of(n, total, header);
    return ADSB_OK;
}

extern "C" int adsb_host_es_integrity(uint32_t tc, uint32_t version, uint32_t supp, uint32_t *nic, uint32_t *rc_dm)
{
    const adsbk::EsIntegrity r = adsbk::es_integrity(tc, version, supp);
    if (nic) *nic = r.nic;
    if (rc_dm) *rc_dm = r.rc_dm;
    return ADSB_OK;
}
