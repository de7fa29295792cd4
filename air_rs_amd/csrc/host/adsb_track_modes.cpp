// adsb_track_modes.cpp -- CPU mirror of the track table's Mode S step: adsb_host_track_modes_of and
// adsb_host_track_modes_merge of include/adsb_host.h.  The per-frame contribution, the empty record and the combine are
// ../adsb_track_modes.h, which the device compiles too; here only the argument checks around them.  No device.
#include "../../../include/adsb_host.h"
#include "../adsb_track_modes.h"

#include <cstring>

extern "C" int adsb_host_track_modes_of(const adsb_modes_rec *rec, double time, adsb_aircraft_modes *one,
                                        uint32_t *accepted)
{
    if (!rec || !one) return ADSB_E_ARG;
    const bool ok = adsbk::modes_accepted(*rec);
    const adsb_aircraft_modes a = ok ? adsbk::modes_one(*rec, time) : adsbk::modes_empty_record();
    std::memcpy(one, &a, sizeof(a));
    if (accepted) *accepted = ok ? 1u : 0u;
    return ADSB_OK;
}

extern "C" int adsb_host_track_modes_merge(adsb_aircraft_modes *into, const adsb_aircraft_modes *later)
{
    if (!into || !later) return ADSB_E_ARG;
    adsb_aircraft_modes a, b;
    std::memcpy(&a, into, sizeof(a));
    std::memcpy(&b, later, sizeof(b));
    adsbk::modes_merge(a, b);
    std::memcpy(into, &a, sizeof(a));
    return ADSB_OK;
}
