// adsb_track_filter.h -- the Kalman filter behind a table's multilaterated fixes: include/adsb_hip.h, "Filtered mlat
// track per aircraft".  One text for the device (adsb_track.hip: filter_operand in one thread per sorted frame,
// filter_step in one thread per segment head, frame after frame) and the CPU mirror (host/adsb_track_filter.cpp): every
// function here is __host__ __device__ under hipcc and plain inline C++ otherwise.  f64 with contraction off.  All
// trigonometry and the one root are in filter_operand; filter_step has only + - x / and compares, so device and mirror
// evaluate the same rounded operations in the same order and agree bit for bit on the same operands.
#ifndef ADSB_TRACK_FILTER_H
#define ADSB_TRACK_FILTER_H

#include "adsb_fix.h"
#include "adsb_mlat.h"

namespace adsbk {

static_assert(sizeof(adsb_track_filter_cfg) == 96 && sizeof(adsb_aircraft_filter) == 192 &&
                  sizeof(adsb_frame_filter) == 32 && sizeof(adsb_filter_operand) == 64,
              "filter records");

constexpr double kFilterMaxLatitude = 89.0;
constexpr double kFilterMinHeightM = -1000.0, kFilterMaxHeightM = 100000.0;
constexpr double kFilterHuge = 1.7976931348623157e308; // DBL_MAX: |x| <= this iff x is finite

// The cfg a reserve keeps: 0 takes the default.  false: a field is neither 0 nor finite and > 0, or reserved is not 0
inline bool filter_cfg_resolve(const adsb_track_filter_cfg *in, adsb_track_filter_cfg &out)
{
    const adsb_track_filter_cfg zero{};
    const adsb_track_filter_cfg c = in ? *in : zero;
    const double given[10] = {c.accel_h, c.accel_v, c.range_sigma_m, c.altitude_sigma_m, c.gate, c.reset_gap_s,
                              c.init_speed_sigma_h, c.init_speed_sigma_v, c.max_hdop, c.max_vdop};
    const double dflt[10] = {3.0, 1.5, 30.0, 15.0, 4.0, 30.0, 300.0, 30.0, 20.0, 50.0};
    double use[10];
    for (int k = 0; k < 10; ++k) {
        if (given[k] == 0.0)
            use[k] = dflt[k];
        else if (given[k] > 0.0 && given[k] <= kFilterHuge)
            use[k] = given[k];
        else
            return false; // negative, infinite or NaN
    }
    if (c.reserved != 0) return false;
    out = zero;
    out.accel_h = use[0];
    out.accel_v = use[1];
    out.range_sigma_m = use[2];
    out.altitude_sigma_m = use[3];
    out.gate = use[4];
    out.reset_gap_s = use[5];
    out.init_speed_sigma_h = use[6];
    out.init_speed_sigma_v = use[7];
    out.max_hdop = use[8];
    out.max_vdop = use[9];
    out.max_outliers = c.max_outliers ? c.max_outliers : 3u;
    out.min_run = c.min_run ? c.min_run : 4u;
    return true;
}

ADSB_HD inline bool filter_finite(double x) { return (x < 0.0 ? -x : x) <= kFilterHuge; }

// One frame's operand (the header's PER FRAME).  c: a resolved cfg; counted: the frame's slot is not kTrackUntracked.
ADSB_HD inline adsb_filter_operand filter_operand(const adsb_track_filter_cfg &c, const adsb_mlat_fix &fix, double time,
                                                  bool counted)
{
#pragma clang fp contract(off)
    adsb_filter_operand o;
    __builtin_memset(&o, 0, sizeof(o));
    if (!counted || !(fix.flags & ADSB_MLAT_VALID)) return o;
    const double lat = fix.latitude, lon = fix.longitude, h = fix.height_m;
    const double hdop = (double)fix.hdop, vdop = (double)fix.vdop, res = (double)fix.residual_rms_m;
    if (!((lat < 0.0 ? -lat : lat) <= kFilterMaxLatitude) || !filter_finite(lon)) return o;
    if (!(h >= kFilterMinHeightM && h <= kFilterMaxHeightM)) return o;
    if (!(hdop > 0.0 && hdop <= c.max_hdop)) return o;
    const double sr = res > c.range_sigma_m ? res : c.range_sigma_m;
    const double sh = hdop * sr, var_h = sh * sh;
    if (!filter_finite(var_h)) return o;
    const bool altitude = (fix.flags & ADSB_MLAT_ALTITUDE) != 0;
    const double sv = vdop * sr;
    double var_v = altitude ? c.altitude_sigma_m * c.altitude_sigma_m : sv * sv;
    const bool height = filter_finite(var_v) && (altitude || (vdop > 0.0 && vdop <= c.max_vdop));
    if (!height) {
        const double s0 = c.max_vdop * sr;
        var_v = s0 * s0;
    }
    const double phi = lat * kMlatRad;
    const double sp = sin(phi), cp = cos(phi);
    const double w2 = 1.0 - kMlatE2 * (sp * sp);
    const double w = sqrt(w2);
    const double m = kMlatA * (1.0 - kMlatE2) / (w2 * w), nn = kMlatA / w;
    o.time = time;
    o.latitude = lat;
    o.longitude = lon;
    o.rn = (m + h) * kMlatRad;
    o.re = (nn + h) * cp * kMlatRad;
    o.var_h = var_h;
    o.var_v = var_v;
    o.height_m = (float)h;
    o.flags = ADSB_TRACK_FILTER_USABLE | (height ? ADSB_TRACK_FILTER_HEIGHT : 0u);
    return o;
}

// The 192 bytes of a filter record as words, for stores and moves
struct FilterWords {
    uint64_t w[24];
};

// The empty record: time NaN, all else zero
ADSB_HD inline FilterWords filter_empty()
{
    adsb_aircraft_filter a;
    __builtin_memset(&a, 0, sizeof(a));
    a.time = __builtin_nan("");
    FilterWords o;
    __builtin_memcpy(&o, &a, sizeof(o));
    return o;
}

ADSB_HD inline uint32_t filter_inc(uint32_t x) { return x == 0xFFFFFFFFu ? x : x + 1u; }

ADSB_HD inline double filter_wrap(double deg)
{
    if (deg > 180.0) return deg - 360.0;
    if (deg < -180.0) return deg + 360.0;
    return deg;
}

// START: the state begins at this fix; the counts stay
ADSB_HD inline void filter_start(const adsb_track_filter_cfg &c, adsb_aircraft_filter &a, const adsb_filter_operand &o)
{
#pragma clang fp contract(off)
    const double vh = c.init_speed_sigma_h * c.init_speed_sigma_h, vv = c.init_speed_sigma_v * c.init_speed_sigma_v;
    a.time = o.time;
    a.latitude = o.latitude;
    a.longitude = o.longitude;
    a.height_m = (double)o.height_m;
    a.v_north = a.v_east = a.v_up = 0.0;
    a.p_north[0] = o.var_h, a.p_north[1] = 0.0, a.p_north[2] = vh;
    a.p_east[0] = o.var_h, a.p_east[1] = 0.0, a.p_east[2] = vh;
    a.p_up[0] = o.var_v, a.p_up[1] = 0.0, a.p_up[2] = vv;
    a.run = 1;
    a.outliers_run = 0;
    a.flags = ADSB_TRACK_FILTER_RUNNING | (o.flags & ADSB_TRACK_FILTER_HEIGHT);
}

// One axis after the predict step: displacement and covariance
struct FilterAxis {
    double p, pp, pv, vv;
};

ADSB_HD inline FilterAxis filter_predict(double v, const double P[3], double q, double dt)
{
#pragma clang fp contract(off)
    const double dt2 = dt * dt;
    FilterAxis x;
    x.p = v * dt;
    x.pp = P[0] + 2.0 * dt * P[1] + dt2 * P[2] + q * (dt2 * dt2) / 4.0;
    x.pv = P[1] + dt * P[2] + q * (dt2 * dt) / 2.0;
    x.vv = P[2] + q * dt2;
    return x;
}

// The update of one measured axis: innovation y, S = x.pp + var; returns the displacement d
ADSB_HD inline double filter_apply(const FilterAxis &x, double y, double s, double &v, double P[3])
{
#pragma clang fp contract(off)
    const double kp = x.pp / s, kv = x.pv / s;
    v = v + kv * y;
    P[0] = (1.0 - kp) * x.pp;
    P[1] = (1.0 - kp) * x.pv;
    P[2] = x.vv - kv * x.pv;
    return x.p + kp * y;
}

// One frame of the walk (the header's PER AIRCRAFT): the record after it, and its per-frame output.  An operand that is
// not usable changes nothing and gives 32 zero bytes.
ADSB_HD inline void filter_step(const adsb_track_filter_cfg &c, adsb_aircraft_filter &a, const adsb_filter_operand &o,
                                adsb_frame_filter &f)
{
#pragma clang fp contract(off)
    __builtin_memset(&f, 0, sizeof(f));
    if (!(o.flags & ADSB_TRACK_FILTER_USABLE)) return;
    uint32_t flags = ADSB_TRACK_FILTER_USABLE;
    double nis = 0.0;
    bool start = !(a.flags & ADSB_TRACK_FILTER_RUNNING);
    if (!start) {
        const double dt = o.time - a.time;
        if (!(dt >= 0.0)) {
            flags |= ADSB_TRACK_FILTER_SKIPPED;
            a.n_skipped = filter_inc(a.n_skipped);
        } else if (dt > c.reset_gap_s) {
            flags |= ADSB_TRACK_FILTER_RESET;
            a.n_reset = filter_inc(a.n_reset);
            start = true;
        } else {
            const double qh = c.accel_h * c.accel_h, qv = c.accel_v * c.accel_v;
            const FilterAxis xn = filter_predict(a.v_north, a.p_north, qh, dt);
            const FilterAxis xe = filter_predict(a.v_east, a.p_east, qh, dt);
            const double yn = (o.latitude - a.latitude) * o.rn - xn.p;
            const double ye = filter_wrap(o.longitude - a.longitude) * o.re - xe.p;
            const double sn = xn.pp + o.var_h, se = xe.pp + o.var_h;
            nis = yn * yn / sn + ye * ye / se;
            a.last_nis = (float)nis;
            if (nis > c.gate * c.gate) {
                flags |= ADSB_TRACK_FILTER_OUTLIER;
                a.n_outlier = filter_inc(a.n_outlier);
                a.outliers_run = filter_inc(a.outliers_run);
                if (a.outliers_run >= c.max_outliers) {
                    flags |= ADSB_TRACK_FILTER_RESET;
                    a.n_reset = filter_inc(a.n_reset);
                    start = true;
                }
            } else {
                const FilterAxis xu = filter_predict(a.v_up, a.p_up, qv, dt);
                const double dn = filter_apply(xn, yn, sn, a.v_north, a.p_north);
                const double de = filter_apply(xe, ye, se, a.v_east, a.p_east);
                double du = xu.p;
                if (o.flags & ADSB_TRACK_FILTER_HEIGHT) {
                    const double yu = ((double)o.height_m - a.height_m) - xu.p;
                    du = filter_apply(xu, yu, xu.pp + o.var_v, a.v_up, a.p_up);
                    a.flags |= ADSB_TRACK_FILTER_HEIGHT;
                } else {
                    a.p_up[0] = xu.pp, a.p_up[1] = xu.pv, a.p_up[2] = xu.vv;
                }
                a.latitude = a.latitude + dn / o.rn;
                a.longitude = filter_wrap(a.longitude + de / o.re);
                a.height_m = a.height_m + du;
                a.time = o.time;
                a.n_applied = filter_inc(a.n_applied);
                a.run = filter_inc(a.run);
                a.outliers_run = 0;
                flags |= ADSB_TRACK_FILTER_APPLIED;
            }
        }
    }
    if (start) {
        filter_start(c, a, o);
        flags |= ADSB_TRACK_FILTER_INIT;
    }
    if (a.run >= c.min_run)
        a.flags |= ADSB_TRACK_FILTER_VELOCITY;
    else
        a.flags &= ~ADSB_TRACK_FILTER_VELOCITY;
    f.latitude = a.latitude;
    f.longitude = a.longitude;
    f.height_m = (float)a.height_m;
    f.nis = (float)nis;
    f.flags = flags;
}

} // namespace adsbk
#endif
