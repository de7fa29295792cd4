// adsb_fix.h -- the locally unambiguous CPR decode of ONE position message against a known reference position (the
// receiver site), with range and bearing from the site: include/adsb_hip.h, "Positions from single messages".  One text
// for the device (adsb_track.hip, one thread per frame) and the CPU mirror (host/adsb_fix.cpp, adsb_host_fix_of): every
// function here is __host__ __device__ under hipcc and plain inline C++ otherwise.  All arithmetic is f64 with
// contraction off, so both sides evaluate the same rounded products; what is left to differ is the last bit of the
// two math libraries' sin / cos / asin / acos / atan2.
#ifndef ADSB_FIX_H
#define ADSB_FIX_H

#include <math.h>
#include <stdint.h>

#include "../../include/adsb_hip.h"

#if defined(__HIPCC__)
#define ADSB_HD __host__ __device__
#else
#define ADSB_HD
#endif

namespace adsbk {

ADSB_HD inline uint32_t floor_as_u32(double x) // Rust `x.floor() as u32`: saturating, NaN -> 0
{
    const double f = floor(x);
    if (!(f >= 0.0)) return 0u;
    if (f >= 4294967295.0) return 4294967295u;
    return (uint32_t)f;
}

ADSB_HD inline uint32_t calc_num_zones(double lat) // cpr.rs:39-54
{
    if (lat == 0.0) return 59;
    if (lat == 87.0 || lat == -87.0) return 2;
    if (lat < -87.0 || lat > 87.0) return 1;
    const double pi = 3.14159265358979323846264338327950288;
    const double int1 = 1.0 - cos(pi / 30.0);
    const double int2 = cos(pi / 180.0 * lat);
    const double int3 = (2.0 * pi) / acos(1.0 - (int1 / (int2 * int2)));
    return floor_as_u32(int3);
}

// ME bits [first, first + width) of the 56-bit ME field (bit 0 = the top bit of frame byte 4)
ADSB_HD inline uint32_t me_bits(uint64_t me, int first, int width)
{
    return (uint32_t)(me >> (56 - first - width)) & ((1u << width) - 1u);
}

// What a frame's decode leaves beside its adsb_frame_fix: the rest of what the aircraft's adsb_fix takes from the
// newest accepted message.  16 bytes per frame.
struct FixRem {
    float ground_speed_kt, track_deg; // surface only; 0 unless flagged in adsb_frame_fix.flags
    int32_t altitude;                 // feet; 0 unless ADSB_FIX_ALT
    uint8_t type_code, cpr_odd;
    uint16_t pad;
};
static_assert(sizeof(FixRem) == 16, "FixRem: the header's memory figures assume 16 bytes");
static_assert(sizeof(adsb_fix) == 64 && sizeof(adsb_frame_fix) == 32 && sizeof(adsb_site) == 24, "fix records");

ADSB_HD inline double fix_mod(double a, double b)
{
#pragma clang fp contract(off)
    return a - b * floor(a / b);
}

// Surface movement (ME bits 5-11) -> ground speed in knots; false: no speed (0, and 125-127 reserved)
ADSB_HD inline bool fix_movement_kt(uint32_t m, double &kt)
{
    if (m == 0 || m >= 125) return false;
    if (m == 1) kt = 0.0;
    else if (m <= 8) kt = 0.125 + (double)(m - 2) * 0.125;
    else if (m <= 12) kt = 1.0 + (double)(m - 9) * 0.25;
    else if (m <= 38) kt = 2.0 + (double)(m - 13) * 0.5;
    else if (m <= 93) kt = 15.0 + (double)(m - 39);
    else if (m <= 108) kt = 70.0 + (double)(m - 94) * 2.0;
    else if (m <= 123) kt = 100.0 + (double)(m - 109) * 5.0;
    else kt = 175.0;
    return true;
}

// One frame against one site.  f.icao is always set.  Not a position message (DF 17, TC 5-8, 9-18, 20-22): everything
// else zero.  Rejected (|lat| > 90, or farther than the site's limit): f.flags = ADSB_FIX_REJECTED (| ADSB_FIX_SURFACE)
// and everything else zero.  Accepted: f.flags = ADSB_FIX_VALID | ..., f and r filled.  range_f64: the accepted frame's
// range from the site in NM before its one rounding to f32 (0 otherwise), for adsb_track_mlat.h.
ADSB_HD inline void fix_decode(const adsb_site &site, const uint8_t *bytes, adsb_frame_fix &f, FixRem &r,
                               double &range_f64)
{
#pragma clang fp contract(off)
    f.latitude = 0.0;
    f.longitude = 0.0;
    f.range_nm = 0.0f;
    f.bearing_deg = 0.0f;
    f.icao = (uint32_t)bytes[1] << 16 | (uint32_t)bytes[2] << 8 | bytes[3];
    f.flags = 0;
    range_f64 = 0.0;
    r.ground_speed_kt = 0.0f;
    r.track_deg = 0.0f;
    r.altitude = 0;
    r.type_code = 0;
    r.cpr_odd = 0;
    r.pad = 0;
    if ((bytes[0] >> 3) != 17) return;
    uint64_t me = 0;
    for (int k = 4; k < 11; ++k) me = me << 8 | bytes[k];
    const uint32_t tc = me_bits(me, 0, 5);
    const bool surface = tc >= 5 && tc <= 8;
    if (!surface && !(tc >= 9 && tc <= 18) && !(tc >= 20 && tc <= 22)) return;
    const uint32_t odd = me_bits(me, 21, 1);
    const double y = (double)me_bits(me, 22, 17) / 131072.0, x = (double)me_bits(me, 39, 17) / 131072.0;
    const double span = surface ? 90.0 : 360.0;
    const uint32_t kind = surface ? ADSB_FIX_SURFACE : 0u;
    f.flags = ADSB_FIX_REJECTED | kind; // until accepted

    const double d_lat = span / (double)(60u - odd);
    const double j = floor(site.latitude / d_lat) + floor(0.5 + fix_mod(site.latitude, d_lat) / d_lat - y);
    const double lat = d_lat * (j + y);
    if (!(fabs(lat) <= 90.0)) return;
    const uint32_t nl = calc_num_zones(lat);
    const double d_lon = span / (double)(nl > odd ? nl - odd : 1u); // max(NL - i, 1); NL >= 1
    const double m = floor(site.longitude / d_lon) + floor(0.5 + fix_mod(site.longitude, d_lon) / d_lon - x);
    double lon = d_lon * (m + x);
    while (lon < -180.0) lon += 360.0; // cpr.rs:27-31
    while (lon > 180.0) lon -= 360.0;

    const double pi = 3.14159265358979323846264338327950288, rad = pi / 180.0;
    const double p1 = site.latitude * rad, p2 = lat * rad, dl = (lon - site.longitude) * rad;
    const double sp = sin((p2 - p1) / 2.0), sl = sin(dl / 2.0);
    const double h = sp * sp + cos(p1) * cos(p2) * (sl * sl);
    const double root = sqrt(h);
    const double range = 2.0 * 3440.065 * asin(root < 1.0 ? root : 1.0);
    const double limit = surface && site.max_range_nm > 45.0 ? 45.0 : site.max_range_nm;
    if (!(range <= limit)) return;
    double bearing = atan2(sin(dl) * cos(p2), cos(p1) * sin(p2) - sin(p1) * cos(p2) * cos(dl)) * 180.0 / pi;
    if (bearing < 0.0) bearing += 360.0;
    if (bearing >= 360.0) bearing -= 360.0;

    uint32_t flags = ADSB_FIX_VALID | kind;
    if (surface) {
        double kt = 0.0;
        if (fix_movement_kt(me_bits(me, 5, 7), kt)) {
            r.ground_speed_kt = (float)kt;
            flags |= ADSB_FIX_SPEED;
        }
        if (me_bits(me, 12, 1)) {
            r.track_deg = (float)((double)me_bits(me, 13, 7) * 360.0 / 128.0);
            flags |= ADSB_FIX_TRACK;
        }
    } else if (tc <= 18) { // the field decode's altitude (msgs.rs:70-75); TC 20-22 carry GNSS height: none here
        const int code = (int)(me_bits(me, 8, 7) << 4 | me_bits(me, 16, 4));
        r.altitude = code * (me_bits(me, 15, 1) ? 25 : 100) - 1000;
        flags |= ADSB_FIX_ALT;
    }
    r.type_code = (uint8_t)tc;
    r.cpr_odd = (uint8_t)odd;
    f.latitude = lat;
    f.longitude = lon;
    f.range_nm = (float)range;
    range_f64 = range;
    f.bearing_deg = (float)bearing;
    if (f.bearing_deg >= 360.0f) f.bearing_deg = 0.0f; // the one rounding lifts a bearing within 1.5e-5 below 360 to 360
    f.flags = flags;
}

ADSB_HD inline void fix_decode(const adsb_site &site, const uint8_t *bytes, adsb_frame_fix &f, FixRem &r)
{
    double range;
    fix_decode(site, bytes, f, r, range);
}

// What a fixes reserve accepts (a NaN fails every comparison)
ADSB_HD inline bool fix_site_ok(const adsb_site &s)
{
    return s.latitude >= -90.0 && s.latitude <= 90.0 && s.longitude >= -180.0 && s.longitude <= 180.0 &&
           s.max_range_nm > 0.0 && s.max_range_nm <= 180.0;
}

// The 64 bytes of a fix, for stores and moves that must carry the record's tail padding too
struct FixWords {
    uint64_t w[8];
};

// The empty fix: time NaN, all else zero (padding included)
ADSB_HD inline FixWords fix_empty()
{
    adsb_fix a;
    __builtin_memset(&a, 0, sizeof(a));
    a.time = __builtin_nan("");
    FixWords o;
    __builtin_memcpy(&o, &a, sizeof(o));
    return o;
}

// An accepted message becomes the aircraft's fix: everything but the two counts
ADSB_HD inline void fix_take(adsb_fix &a, const adsb_frame_fix &f, const FixRem &r, double time)
{
    a.time = time;
    a.latitude = f.latitude;
    a.longitude = f.longitude;
    a.range_nm = f.range_nm;
    a.bearing_deg = f.bearing_deg;
    a.ground_speed_kt = r.ground_speed_kt;
    a.track_deg = r.track_deg;
    a.altitude = r.altitude;
    a.type_code = r.type_code;
    a.flags = (uint8_t)f.flags;
    a.cpr_odd = r.cpr_odd;
    a.reserved8 = 0;
    a.reserved = 0;
}

} // namespace adsbk
#endif
