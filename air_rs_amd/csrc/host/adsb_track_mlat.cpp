// adsb_track_mlat.cpp -- CPU mirror of the track table's per-frame mlat step: adsb_host_track_mlat_of of include/
// adsb_host.h.  The per-frame text is ../adsb_track_mlat.h, which the device compiles too; here only the one-frame merge
// around it.  No device.
#include "../../../include/adsb_host.h"
#include "../adsb_track_mlat.h"

#include <cmath>
#include <cstring>

extern "C" int adsb_host_track_mlat_of(double max_disagreement_m, const uint8_t bytes[14], const adsb_mlat_fix *fix,
                                       double time, adsb_aircraft_mlat *out, uint32_t *frame_flags,
                                       float *disagreement_m)
{
    if (!bytes || !fix || !out || !std::isfinite(max_disagreement_m) || !(max_disagreement_m > 0.0)) return ADSB_E_ARG;
    const adsbk::MlatFrame m = adsbk::mlat_frame(max_disagreement_m, bytes, *fix);
    const adsbk::MlatWords empty = adsbk::mlat_empty();
    adsb_aircraft_mlat a;
    std::memcpy(&a, &empty, sizeof(a));
    if (m.flags & ADSB_TRACK_MLAT_CHECKED) {
        a.last_disagreement_m = a.max_disagreement_m = m.disagreement_m;
        a.flags |= ADSB_TRACK_MLAT_CHECKED;
        a.n_checked = 1;
        a.n_disagree = (m.flags & ADSB_TRACK_MLAT_DISAGREE) ? 1u : 0u;
    }
    if (m.flags & ADSB_TRACK_MLAT_VALID) {
        adsbk::mlat_take(a, *fix, time);
        a.n_valid = 1;
    }
    a.n_attempted = m.attempted;
    std::memcpy(out, &a, sizeof(a));
    if (frame_flags) *frame_flags = m.flags;
    if (disagreement_m) *disagreement_m = m.disagreement_m;
    return ADSB_OK;
}
