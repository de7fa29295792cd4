// adsb_track_es.cpp -- CPU mirror of the track table's extended squitter step: adsb_host_es_resolve,
// adsb_host_track_es_of and adsb_host_track_es_merge of include/adsb_host.h.  The resolution, the per-frame
// contribution, the empty record and the combine are ../adsb_track_es.h, which the device compiles too; here only the
// argument checks around them.  No device.
#include "../../../include/adsb_host.h"
#include "../adsb_track_es.h"

#include <cstring>

extern "C" int adsb_host_es_resolve(const adsb_es_rec *rec, double time, const adsb_aircraft_es *held,
                                    const adsb_es_track_cfg *cfg, adsb_frame_integrity *out)
{
    if (!rec || !out) return ADSB_E_ARG;
    const double max_age_s = cfg ? cfg->max_age_s : 60.0;
    if (!(max_age_s >= 0.0)) return ADSB_E_ARG;
    adsb_es_rec r;
    std::memcpy(&r, rec, sizeof(r));
    adsbk::EsKnown k = adsbk::es_known_none();
    if (held) {
        adsb_aircraft_es a;
        std::memcpy(&a, held, sizeof(a));
        k = adsbk::es_known_of_record(a);
    }
    const adsb_frame_integrity o = adsbk::es_track_resolve(r, time, k, max_age_s);
    std::memcpy(out, &o, sizeof(o));
    return ADSB_OK;
}

extern "C" int adsb_host_track_es_of(const adsb_es_rec *rec, const adsb_frame_integrity *integrity, double time,
                                     adsb_aircraft_es *one)
{
    if (!rec || !integrity || !one) return ADSB_E_ARG;
    adsb_es_rec r;
    adsb_frame_integrity f;
    std::memcpy(&r, rec, sizeof(r));
    std::memcpy(&f, integrity, sizeof(f));
    const adsb_aircraft_es a = adsbk::es_track_one(r, f, time);
    std::memcpy(one, &a, sizeof(a));
    return ADSB_OK;
}

extern "C" int adsb_host_track_es_merge(adsb_aircraft_es *into, const adsb_aircraft_es *later)
{
    if (!into || !later) return ADSB_E_ARG;
    adsb_aircraft_es a, b;
    std::memcpy(&a, into, sizeof(a));
    std::memcpy(&b, later, sizeof(b));
    adsbk::es_track_merge(a, b);
    std::memcpy(into, &a, sizeof(a));
    return ADSB_OK;
}
