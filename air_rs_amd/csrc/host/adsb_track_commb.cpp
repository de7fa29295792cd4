// adsb_track_commb.cpp -- CPU mirror of the track table's Comm-B step: adsb_host_commb_settle,
// adsb_host_track_commb_of and adsb_host_track_commb_merge of include/adsb_host.h.  The reference, the checks, the
// decision, the per-frame contribution, the empty record and the combine are ../adsb_track_commb.h, which the device
// compiles too; here only the argument checks around them.  No device.
#include "../../../include/adsb_host.h"
#include "../adsb_track_commb.h"

#include <cstring>

extern "C" int adsb_host_commb_settle(const uint8_t bytes[14], const adsb_commb_rec *rec, const adsb_velocity *reference,
                                      double time, const adsb_commb_settle_cfg *cfg, adsb_commb_rec *out)
{
    if (!bytes || !rec || !out) return ADSB_E_ARG;
    const adsb_commb_settle_cfg use = cfg ? *cfg : adsb_commb_settle_cfg{10.0, 40u, 1000u};
    if (!(use.max_age_s >= 0.0)) return ADSB_E_ARG;
    adsb_commb_rec r;
    std::memcpy(&r, rec, sizeof(r));
    adsbk::CommbRef v = adsbk::commb_ref_none();
    if (reference) {
        adsb_velocity held;
        std::memcpy(&held, reference, sizeof(held));
        v = adsbk::commb_ref_of_velocity(held);
    }
    const adsb_commb_rec o = adsbk::commb_settle(adsbk::modes_bytes(bytes), r, v, time, use);
    std::memcpy(out, &o, sizeof(o));
    return ADSB_OK;
}

extern "C" int adsb_host_commb_reference(const uint8_t bytes[14], double time, adsb_velocity *reference)
{
    if (!bytes || !reference) return ADSB_E_ARG;
    const adsbk::CommbRef v = adsbk::commb_ref_of_frame(adsbk::modes_bytes(bytes), time);
    adsb_velocity o{};
    o.time = v.time;
    o.subtype = (uint8_t)v.subtype;
    o.flags = (uint8_t)v.flags;
    o.vertical_rate_fpm = v.vr;
    o.v_ew_kt = (int16_t)v.ew;
    o.v_ns_kt = (int16_t)v.ns;
    o.airspeed_tas = (uint8_t)v.tas;
    if (v.subtype >= 3) {
        o.speed_kt = (float)v.speed;
        o.direction_deg = (float)((double)v.h10 * 45.0 / 128.0);
    }
    std::memcpy(reference, &o, sizeof(o));
    return ADSB_OK;
}

extern "C" int adsb_host_track_commb_of(const adsb_commb_rec *rec, double time, adsb_aircraft_commb *one)
{
    if (!rec || !one) return ADSB_E_ARG;
    adsb_commb_rec r;
    std::memcpy(&r, rec, sizeof(r));
    const adsb_aircraft_commb a =
        r.state != ADSB_COMMB_NOT_COMMB ? adsbk::commb_one(r, time) : adsbk::commb_empty_record();
    std::memcpy(one, &a, sizeof(a));
    return ADSB_OK;
}

extern "C" int adsb_host_track_commb_merge(adsb_aircraft_commb *into, const adsb_aircraft_commb *later)
{
    if (!into || !later) return ADSB_E_ARG;
    adsb_aircraft_commb a, b;
    std::memcpy(&a, into, sizeof(a));
    std::memcpy(&b, later, sizeof(b));
    adsbk::commb_merge(a, b);
    std::memcpy(into, &a, sizeof(a));
    return ADSB_OK;
}
