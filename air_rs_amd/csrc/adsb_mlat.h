// adsb_mlat.h -- multilateration of one correlated message (include/adsb_hip.h, "Multilaterate"): geodetic <-> ECEF, the
// altitude decode, the time difference and rho of a reception, its residual and Jacobian row, the 15 sums and their
// butterfly order, the 4 x 4 factorisation, the Levenberg-Marquardt step rule and its two stages, the dilutions and the
// flag logic.  One text for the device (adsb_mlat.hip, 16 lanes per message) and the CPU mirror (host/adsb_mlat.cpp,
// adsb_host_multilaterate, a walk over messages): every function here is __host__ __device__ under hipcc and plain inline
// C++ otherwise.  What the two sides supply is `Eval`: the folded sums of the range rows at a point, which the device
// takes from its lanes' partial sums and the mirror from 16 partial sums of its own, folded by mlat_fold16 in the same
// order.  All arithmetic is f64 with contraction off, so both sides evaluate the same rounded operations in the same
// order; what is left to differ is the last bit of the math libraries' atan2 / sin / cos in the height formula.
#ifndef ADSB_MLAT_H
#define ADSB_MLAT_H

#include <math.h>
#include <stdint.h>

#include "../../include/adsb_hip.h"

#if defined(__HIPCC__)
#define ADSB_MLAT_HD __host__ __device__
#else
#define ADSB_MLAT_HD
#endif

namespace adsbk {

constexpr uint32_t kMlatLanes = 16;        // partial sums of every sum over receptions; the device's lanes per message
constexpr uint32_t kMlatMaxReceivers = 256;
constexpr double kMlatC = ADSB_MLAT_C;
constexpr double kMlatA = 6378137.0, kMlatF = 1.0 / 298.257223563;
constexpr double kMlatB = kMlatA * (1.0 - kMlatF);
constexpr double kMlatE2 = kMlatF * (2.0 - kMlatF);                                   // first eccentricity squared
constexpr double kMlatEp2 = (kMlatA * kMlatA - kMlatB * kMlatB) / (kMlatB * kMlatB);  // second
constexpr double kMlatLambda0 = 1e-3, kMlatLambdaMin = 1e-12, kMlatLambdaMax = 1e12;
constexpr double kMlatPivot = 1e-12;       // a pivot must exceed this times its diagonal entry
constexpr double kMlatRad = 3.14159265358979323846264338327950288 / 180.0;

// A receiver as the solver sees it: ECEF metres, computed on the host by mlat_station_of in both paths, and its clock.
struct MlatStation {
    double x, y, z, clock;
};
static_assert(sizeof(MlatStation) == 32 && sizeof(adsb_mlat_receiver) == 32 && sizeof(adsb_mlat_fix) == 64 &&
                  sizeof(adsb_mlat_cfg) == 64 && sizeof(adsb_mlat_header) == 32,
              "multilaterate records");

// The cfg with its defaults filled in.
struct MlatParams {
    uint32_t time_source, flags, min_receivers, max_iterations;
    double seconds_per_tick, step_tol_m, max_residual_m, max_range_m, default_altitude_m;
};

// What the entry points accept (a NaN fails every comparison)
inline bool mlat_cfg_ok(const adsb_mlat_cfg &c)
{
    if (c.time_source > ADSB_MLAT_TIME_TICKS || (c.flags & ~ADSB_MLAT_USE_ALTITUDE) != 0) return false;
    if (c.min_receivers > kMlatMaxReceivers || c.max_iterations > 1000u) return false;
    const bool spt = c.time_source == ADSB_MLAT_TIME_TICKS ? c.seconds_per_tick >= 0.0 : c.seconds_per_tick > 0.0;
    return spt && c.seconds_per_tick <= 1.0 && c.step_tol_m >= 0.0 && c.step_tol_m <= 1e6 && c.max_residual_m >= 0.0 &&
           c.max_residual_m <= 1e12 && c.max_range_m >= 0.0 && c.max_range_m <= 1e8 && c.default_altitude_m >= -1000.0 &&
           c.default_altitude_m <= 100000.0;
}

inline bool mlat_receiver_ok(const adsb_mlat_receiver &r)
{
    return r.latitude >= -90.0 && r.latitude <= 90.0 && r.longitude >= -180.0 && r.longitude <= 180.0 &&
           r.height_m >= -1000.0 && r.height_m <= 100000.0 && r.clock_offset_s >= -1e6 && r.clock_offset_s <= 1e6;
}

inline MlatParams mlat_params_of(const adsb_mlat_cfg &c)
{
    MlatParams p;
    p.time_source = c.time_source;
    p.flags = c.flags;
    p.min_receivers = c.min_receivers;
    p.max_iterations = c.max_iterations ? c.max_iterations : 24u;
    p.seconds_per_tick = c.seconds_per_tick != 0.0 ? c.seconds_per_tick : 1.0 / 12e6;
    p.step_tol_m = c.step_tol_m != 0.0 ? c.step_tol_m : 0.01;
    p.max_residual_m = c.max_residual_m;
    p.max_range_m = c.max_range_m != 0.0 ? c.max_range_m : 500e3;
    p.default_altitude_m = c.default_altitude_m != 0.0 ? c.default_altitude_m : 10000.0;
    return p;
}

// geodetic (degrees, metres) -> ECEF.  Host only: both paths take their stations from here.
inline MlatStation mlat_station_of(const adsb_mlat_receiver &r)
{
#pragma clang fp contract(off)
    const double phi = r.latitude * kMlatRad, lam = r.longitude * kMlatRad;
    const double sp = sin(phi), cp = cos(phi);
    const double n = kMlatA / sqrt(1.0 - kMlatE2 * (sp * sp));
    MlatStation s;
    s.x = (n + r.height_m) * cp * cos(lam);
    s.y = (n + r.height_m) * cp * sin(lam);
    s.z = (n * (1.0 - kMlatE2) + r.height_m) * sp;
    s.clock = r.clock_offset_s;
    return s;
}

// ECEF -> height and the ellipsoid normal (Bowring, two refinement steps), with the trigonometry of the position kept
// for the output conversion.
struct MlatGeo {
    double h, nx, ny, nz; // height; the normal (cos phi cos lambda, cos phi sin lambda, sin phi)
    double phi;           // radians
    double cl, sl;        // cos / sin lambda
};

ADSB_MLAT_HD inline MlatGeo mlat_geodetic(double x, double y, double z)
{
#pragma clang fp contract(off)
    MlatGeo g;
    const double p = sqrt(x * x + y * y);
    g.cl = p > 0.0 ? x / p : 1.0;
    g.sl = p > 0.0 ? y / p : 0.0;
    double beta = atan2(kMlatA * z, kMlatB * p);
    double phi = 0.0;
    for (int k = 0; k < 2; ++k) {
        const double sb = sin(beta), cb = cos(beta);
        phi = atan2(z + kMlatEp2 * kMlatB * (sb * sb * sb), p - kMlatE2 * kMlatA * (cb * cb * cb));
        beta = atan2(kMlatB * sin(phi), kMlatA * cos(phi));
    }
    const double sp = sin(phi), cp = cos(phi);
    g.phi = phi;
    g.h = p * cp + z * sp - kMlatA * sqrt(1.0 - kMlatE2 * (sp * sp));
    g.nx = cp * g.cl;
    g.ny = cp * g.sl;
    g.nz = sp;
    return g;
}

// The altitude a message carries, in metres: DF17/18, type code 9-18, a non-zero code with the 25 ft Q bit.
ADSB_MLAT_HD inline bool mlat_altitude_of(const uint8_t *bytes, double &alt_m)
{
#pragma clang fp contract(off)
    const uint32_t df = bytes[0] >> 3, tc = bytes[4] >> 3;
    if ((df != 17u && df != 18u) || tc < 9u || tc > 18u) return false;
    const uint32_t code = (uint32_t)bytes[5] << 4 | (uint32_t)bytes[6] >> 4; // ME bits 8-19
    if (code == 0u || !(code & 0x10u)) return false;
    const uint32_t n = (code >> 5) << 4 | (code & 0xFu);
    alt_m = ((double)n * 25.0 - 1000.0) * 0.3048;
    return true;
}

ADSB_MLAT_HD inline uint32_t mlat_need(const MlatParams &p, bool has_alt)
{
    const uint32_t floor_ = has_alt ? 3u : 4u;
    return p.min_receivers > floor_ ? p.min_receivers : floor_;
}

// The integer time difference of a reception against the first used one.
ADSB_MLAT_HD inline int64_t mlat_dticks(uint32_t time_source, uint64_t t, uint64_t t0)
{
    const uint64_t d = t - t0;
    if (time_source == ADSB_MLAT_TIME_TICKS) return (int64_t)(d << 16) >> 16; // mod 2^48, sign-extended
    return (int64_t)d;
}

ADSB_MLAT_HD inline double mlat_rho(const MlatParams &p, uint64_t t, uint64_t t0, double clock, double clock0)
{
#pragma clang fp contract(off)
    return kMlatC * ((double)mlat_dticks(p.time_source, t, t0) * p.seconds_per_tick - (clock - clock0));
}

// The 15 sums: v[0..9] = JtJ's upper triangle (00 01 02 03 11 12 13 22 23 33), v[10..13] = Jtr, v[14] = the cost.
struct MlatSums {
    double v[15];
};

ADSB_MLAT_HD inline void mlat_sums_zero(MlatSums &s)
{
    for (int k = 0; k < 15; ++k) s.v[k] = 0.0;
}

ADSB_MLAT_HD inline void mlat_add_row(MlatSums &s, double j0, double j1, double j2, double j3, double r)
{
#pragma clang fp contract(off)
    s.v[0] += j0 * j0;
    s.v[1] += j0 * j1;
    s.v[2] += j0 * j2;
    s.v[3] += j0 * j3;
    s.v[4] += j1 * j1;
    s.v[5] += j1 * j2;
    s.v[6] += j1 * j3;
    s.v[7] += j2 * j2;
    s.v[8] += j2 * j3;
    s.v[9] += j3 * j3;
    s.v[10] += j0 * r;
    s.v[11] += j1 * r;
    s.v[12] += j2 * r;
    s.v[13] += j3 * r;
    s.v[14] += r * r;
}

ADSB_MLAT_HD inline double mlat_dist(const double *x, double sx, double sy, double sz)
{
#pragma clang fp contract(off)
    const double dx = x[0] - sx, dy = x[1] - sy, dz = x[2] - sz;
    return sqrt(dx * dx + dy * dy + dz * dz);
}

// One used reception at the point x = (p, d): its residual and Jacobian row, added to a partial sum.
ADSB_MLAT_HD inline void mlat_range_row(MlatSums &s, const double *x, double sx, double sy, double sz, double rho)
{
#pragma clang fp contract(off)
    const double dx = x[0] - sx, dy = x[1] - sy, dz = x[2] - sz;
    const double range = sqrt(dx * dx + dy * dy + dz * dz);
    const bool far = range > 0.0;
    mlat_add_row(s, far ? dx / range : 0.0, far ? dy / range : 0.0, far ? dz / range : 0.0, 1.0, range + x[3] - rho);
}

// The butterfly over 16 partial values held in one array (the mirror; the device's lanes do the same with shuffles).
inline double mlat_fold16(const double *partial)
{
#pragma clang fp contract(off)
    double v[kMlatLanes], w[kMlatLanes];
    for (uint32_t l = 0; l < kMlatLanes; ++l) v[l] = partial[l];
    for (uint32_t m = 8; m; m >>= 1) {
        for (uint32_t l = 0; l < kMlatLanes; ++l) w[l] = v[l] + v[l ^ m];
        for (uint32_t l = 0; l < kMlatLanes; ++l) v[l] = w[l];
    }
    return v[0];
}

// L D Lt of the normal matrix with its diagonal scaled by 1 + lambda, in the order x, y, z, d.  false: SINGULAR.
struct MlatFactor {
    double l[4][4], d[4];
};

ADSB_MLAT_HD inline bool mlat_factor(const MlatSums &s, double lambda, MlatFactor &f)
{
#pragma clang fp contract(off)
    const double scale = 1.0 + lambda;
    double m[4][4];
    m[0][0] = s.v[0] * scale;
    m[1][0] = s.v[1];
    m[2][0] = s.v[2];
    m[3][0] = s.v[3];
    m[1][1] = s.v[4] * scale;
    m[2][1] = s.v[5];
    m[3][1] = s.v[6];
    m[2][2] = s.v[7] * scale;
    m[3][2] = s.v[8];
    m[3][3] = s.v[9] * scale;
    bool ok = true;
    for (int j = 0; j < 4; ++j) {
        double d = m[j][j];
        for (int k = 0; k < j; ++k) d -= f.l[j][k] * f.l[j][k] * f.d[k];
        if (!(d > kMlatPivot * m[j][j])) {
            ok = false;
            d = 1.0; // keeps the rest finite; the caller drops the result
        }
        f.d[j] = d;
        for (int i = j + 1; i < 4; ++i) {
            double v = m[i][j];
            for (int k = 0; k < j; ++k) v -= f.l[i][k] * f.l[j][k] * f.d[k];
            f.l[i][j] = v / d;
        }
    }
    return ok;
}

// x of (L D Lt) x = b
ADSB_MLAT_HD inline void mlat_backsolve(const MlatFactor &f, const double *b, double *x)
{
#pragma clang fp contract(off)
    double y[4];
    for (int i = 0; i < 4; ++i) {
        double v = b[i];
        for (int k = 0; k < i; ++k) v -= f.l[i][k] * y[k];
        y[i] = v;
    }
    for (int i = 0; i < 4; ++i) y[i] = y[i] / f.d[i];
    for (int i = 3; i >= 0; --i) {
        double v = y[i];
        for (int k = i + 1; k < 4; ++k) v -= f.l[k][i] * x[k];
        x[i] = v;
    }
}

// The sums of a stage's equations at x: the range rows from `eval` (folded), then the altitude row.
template <class Eval>
ADSB_MLAT_HD inline void mlat_sums_at(Eval &eval, const double *x, bool hold_height, double height, MlatSums &s)
{
    eval(x, s);
    if (hold_height) {
        const MlatGeo g = mlat_geodetic(x[0], x[1], x[2]);
        mlat_add_row(s, g.nx, g.ny, g.nz, 0.0, g.h - height);
    }
}

// One stage of Levenberg-Marquardt from x (updated in place); s: the sums at the returned x.  true: converged.
template <class Eval>
ADSB_MLAT_HD inline bool mlat_stage(const MlatParams &p, Eval &eval, bool hold_height, double height, double *x,
                                    MlatSums &s, uint32_t &iterations, bool &singular)
{
#pragma clang fp contract(off)
    mlat_sums_at(eval, x, hold_height, height, s);
    double lambda = kMlatLambda0;
    for (uint32_t it = 0; it < p.max_iterations; ++it) {
        MlatFactor f;
        if (!mlat_factor(s, lambda, f)) {
            singular = true;
            return false;
        }
        const double b[4] = {-s.v[10], -s.v[11], -s.v[12], -s.v[13]};
        double delta[4];
        mlat_backsolve(f, b, delta);
        ++iterations;
        const double trial[4] = {x[0] + delta[0], x[1] + delta[1], x[2] + delta[2], x[3] + delta[3]};
        MlatSums t;
        mlat_sums_at(eval, trial, hold_height, height, t);
        const double step = sqrt(delta[0] * delta[0] + delta[1] * delta[1] + delta[2] * delta[2]);
        if (t.v[14] <= s.v[14]) { // accepted: the cost does not rise
            for (int k = 0; k < 4; ++k) x[k] = trial[k];
            s = t;
            lambda = lambda / 10.0;
            if (lambda < kMlatLambdaMin) lambda = kMlatLambdaMin;
        } else {
            lambda = lambda * 10.0;
            if (lambda > kMlatLambdaMax) lambda = kMlatLambdaMax;
        }
        if (step < p.step_tol_m) return true;
    }
    return false;
}

ADSB_MLAT_HD inline adsb_mlat_fix mlat_fix_empty(uint32_t flags, uint32_t n_used)
{
    adsb_mlat_fix f;
    f.latitude = f.longitude = f.height_m = f.time_s = 0.0;
    f.residual_rms_m = f.pdop = f.hdop = f.vdop = 0.0f;
    f.n_used = (uint16_t)n_used;
    f.iterations = 0;
    f.flags = flags;
    f.reserved = 0;
    return f;
}

// An attempted message: n_used >= mlat_need.  s0: the station of the first used reception; cen: the used receivers'
// centroid (coordinate sums in the butterfly order, each divided by n_used).
template <class Eval>
ADSB_MLAT_HD inline adsb_mlat_fix mlat_solve_message(const MlatParams &p, uint32_t n_used, bool has_alt, double alt_m,
                                                     const double *s0, const double *cen, Eval &eval)
{
#pragma clang fp contract(off)
    const double height = has_alt ? alt_m : p.default_altitude_m;
    const MlatGeo gc = mlat_geodetic(cen[0], cen[1], cen[2]);
    const double up = height - gc.h;
    double x[4] = {cen[0] + gc.nx * up, cen[1] + gc.ny * up, cen[2] + gc.nz * up, 0.0};
    x[3] = -mlat_dist(x, s0[0], s0[1], s0[2]);
    uint32_t iterations = 0;
    bool singular = false;
    MlatSums s;
    bool converged = mlat_stage(p, eval, true, height, x, s, iterations, singular);
    if (!has_alt && !singular) converged = mlat_stage(p, eval, false, 0.0, x, s, iterations, singular);

    adsb_mlat_fix f = mlat_fix_empty(ADSB_MLAT_ATTEMPTED | (has_alt ? ADSB_MLAT_ALTITUDE : 0u), n_used);
    f.iterations = (uint16_t)iterations;
    // dilutions: the position block of the inverse of the undamped normal matrix at x
    MlatFactor fac;
    if (!singular && !mlat_factor(s, 0.0, fac)) singular = true;
    const MlatGeo g = mlat_geodetic(x[0], x[1], x[2]);
    if (!singular) {
        const double e0[4] = {1.0, 0.0, 0.0, 0.0}, e1[4] = {0.0, 1.0, 0.0, 0.0}, e2[4] = {0.0, 0.0, 1.0, 0.0};
        double c0[4], c1[4], c2[4];
        mlat_backsolve(fac, e0, c0);
        mlat_backsolve(fac, e1, c1);
        mlat_backsolve(fac, e2, c2);
        // east (-sl, cl, 0), north (-sp cl, -sp sl, cp), up = the normal; q(v) = v' Q v
        const double sp = g.nz, cp = cos(g.phi);
        const double ex = -g.sl, ey = g.cl;
        const double nx = -sp * g.cl, ny = -sp * g.sl, nz = cp;
        const double qe = ex * (c0[0] * ex + c1[0] * ey) + ey * (c0[1] * ex + c1[1] * ey);
        const double qn = nx * (c0[0] * nx + c1[0] * ny + c2[0] * nz) + ny * (c0[1] * nx + c1[1] * ny + c2[1] * nz) +
                          nz * (c0[2] * nx + c1[2] * ny + c2[2] * nz);
        const double qu = g.nx * (c0[0] * g.nx + c1[0] * g.ny + c2[0] * g.nz) +
                          g.ny * (c0[1] * g.nx + c1[1] * g.ny + c2[1] * g.nz) +
                          g.nz * (c0[2] * g.nx + c1[2] * g.ny + c2[2] * g.nz);
        const double qh = qe + qn;
        f.pdop = (float)sqrt(c0[0] + c1[1] + c2[2]);
        f.hdop = (float)sqrt(qh > 0.0 ? qh : 0.0);
        f.vdop = (float)sqrt(qu > 0.0 ? qu : 0.0);
    }
    f.latitude = g.phi / kMlatRad;
    f.longitude = atan2(g.sl, g.cl) / kMlatRad;
    f.height_m = g.h;
    f.time_s = x[3] / kMlatC;
    const double rows = (double)(n_used + (has_alt ? 1u : 0u)); // the last stage's equations
    const double rms = sqrt(s.v[14] / rows);
    f.residual_rms_m = (float)rms;
    uint32_t flags = f.flags;
    if (converged) flags |= ADSB_MLAT_CONVERGED;
    if (singular) flags |= ADSB_MLAT_SINGULAR;
    if (p.max_residual_m > 0.0 && !(rms <= p.max_residual_m)) flags |= ADSB_MLAT_REJECTED_RESIDUAL;
    if (!(mlat_dist(x, cen[0], cen[1], cen[2]) <= p.max_range_m)) flags |= ADSB_MLAT_REJECTED_RANGE;
    if (converged && !(flags & (ADSB_MLAT_SINGULAR | ADSB_MLAT_REJECTED_RESIDUAL | ADSB_MLAT_REJECTED_RANGE)))
        flags |= ADSB_MLAT_VALID;
    f.flags = flags;
    return f;
}

// What the header's reduction adds up
struct MlatCount {
    uint64_t n_messages, n_attempted, n_valid, flags;
};

ADSB_MLAT_HD inline MlatCount mlat_count_of(uint32_t fix_flags)
{
    MlatCount c;
    c.n_messages = 1;
    c.n_attempted = (fix_flags & ADSB_MLAT_ATTEMPTED) ? 1 : 0;
    c.n_valid = (fix_flags & ADSB_MLAT_VALID) ? 1 : 0;
    c.flags = (fix_flags & ADSB_MLAT_BAD_INDEX) ? ADSB_MLAT_HDR_BAD_INDEX : 0;
    return c;
}

ADSB_MLAT_HD inline MlatCount mlat_count_add(const MlatCount &a, const MlatCount &b)
{
    MlatCount c;
    c.n_messages = a.n_messages + b.n_messages;
    c.n_attempted = a.n_attempted + b.n_attempted;
    c.n_valid = a.n_valid + b.n_valid;
    c.flags = a.flags | b.flags;
    return c;
}

} // namespace adsbk

#endif
