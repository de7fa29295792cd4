// adsb_track_mlat.h -- what ONE frame and its multilaterated fix contribute to the aircraft's mlat record: include/
// adsb_hip.h, "Multilaterated positions per aircraft".  One text for the device (adsb_track.hip, one thread per frame)
// and the CPU mirror (host/adsb_track_mlat.cpp, adsb_host_track_mlat_of): every function here is __host__ __device__
// under hipcc and plain inline C++ otherwise.  The check is adsb_fix.h's single-message decode with the solved position
// as the site, called and not restated; the one product added to it is f64 with contraction off.
#ifndef ADSB_TRACK_MLAT_H
#define ADSB_TRACK_MLAT_H

#include "adsb_fix.h"

namespace adsbk {

static_assert(sizeof(adsb_aircraft_mlat) == 64 && sizeof(adsb_frame_mlat) == 16 && sizeof(adsb_mlat_fix) == 64,
              "mlat records");

constexpr double kMlatCheckRangeNm = 180.0;  // half an airborne zone: as far as a local decode can be trusted
constexpr double kMlatMetresPerNm = 1852.0;
constexpr float kMlatFarM = 333360.0f;       // 180 NM: what a frame the decode turned away reports

// What a counted frame adds to its aircraft's record, before the merge; all zero for a frame that is not counted
struct MlatFrame {
    float disagreement_m; // 0 unless ADSB_TRACK_MLAT_CHECKED
    uint32_t flags;       // ADSB_TRACK_MLAT_VALID / CHECKED / DISAGREE / FAR, as adsb_frame_mlat.flags
    uint32_t attempted;   // 1: the fix has ADSB_MLAT_ATTEMPTED
};

// One counted frame and its fix.  CHECKED iff the fix is valid, its position is a site a fixes reserve would accept with
// the 180 NM limit, and the frame is an airborne position message (the decode says so: a flags word that is neither 0
// nor ADSB_FIX_SURFACE).
ADSB_HD inline MlatFrame mlat_frame(double max_disagreement_m, const uint8_t *bytes, const adsb_mlat_fix &fix)
{
#pragma clang fp contract(off)
    MlatFrame o;
    o.disagreement_m = 0.0f;
    o.flags = 0;
    o.attempted = (fix.flags & ADSB_MLAT_ATTEMPTED) ? 1u : 0u;
    if (!(fix.flags & ADSB_MLAT_VALID)) return o;
    o.flags = ADSB_TRACK_MLAT_VALID;
    adsb_site site;
    site.latitude = fix.latitude;
    site.longitude = fix.longitude;
    site.max_range_nm = kMlatCheckRangeNm;
    if (!fix_site_ok(site)) return o; // a NaN or a position off the globe: nothing to measure from
    adsb_frame_fix f;
    FixRem r;
    double range_nm;
    fix_decode(site, bytes, f, r, range_nm);
    if (f.flags == 0 || (f.flags & ADSB_FIX_SURFACE)) return o; // no position message, or a surface one
    o.flags |= ADSB_TRACK_MLAT_CHECKED;
    if (f.flags & ADSB_FIX_REJECTED) {
        o.flags |= ADSB_TRACK_MLAT_FAR | ADSB_TRACK_MLAT_DISAGREE;
        o.disagreement_m = kMlatFarM;
        return o;
    }
    const double metres = range_nm * kMlatMetresPerNm;
    if (metres > max_disagreement_m) o.flags |= ADSB_TRACK_MLAT_DISAGREE;
    o.disagreement_m = (float)metres;
    return o;
}

// The 64 bytes of an mlat record as words, for stores and moves
struct MlatWords {
    uint64_t w[8];
};

// The empty record: time NaN, all else zero
ADSB_HD inline MlatWords mlat_empty()
{
    adsb_aircraft_mlat a;
    __builtin_memset(&a, 0, sizeof(a));
    a.time = __builtin_nan("");
    MlatWords o;
    __builtin_memcpy(&o, &a, sizeof(o));
    return o;
}

// A valid fix becomes the aircraft's kept fix: everything but the counts and the check's fields
ADSB_HD inline void mlat_take(adsb_aircraft_mlat &a, const adsb_mlat_fix &fix, double time)
{
    a.time = time;
    a.latitude = fix.latitude;
    a.longitude = fix.longitude;
    a.height_m = (float)fix.height_m;
    a.residual_rms_m = fix.residual_rms_m;
    a.pdop = fix.pdop;
    a.n_used = fix.n_used;
    a.flags = (uint8_t)((a.flags & ADSB_TRACK_MLAT_CHECKED) | ADSB_TRACK_MLAT_VALID |
                        ((fix.flags & ADSB_MLAT_ALTITUDE) ? ADSB_TRACK_MLAT_ALTITUDE : 0u));
    a.reserved = 0;
}

} // namespace adsbk
#endif
