// adsb_clock.h -- receiver clock offsets and drift from position messages (include/adsb_hip.h, "Clock sync"): which
// message gives rows and where it was sent from, a row's y, the pair key, the 64-way sums and their butterfly order, the
// entries of the normal equations, the L D Lt entry and the substitution steps, the residual, the records' fields and
// the apply formula.  One text for the device (adsb_clock.hip) and the CPU mirror (host/adsb_clock.cpp): every function
// here is __host__ __device__ under hipcc and plain inline C++ otherwise.  Times, the integer tick difference and the
// altitude rule are adsb_mlat.h's, called and not restated; the position decode is adsb_fix.h's.  All arithmetic is f64
// with contraction off, so both sides evaluate the same rounded operations in the same order; what is left to differ
// is the last bit of the math libraries' sin / cos / sqrt in the decode, the ECEF point and the ranges.
#ifndef ADSB_CLOCK_H
#define ADSB_CLOCK_H

#include "adsb_clock_records.h"
#include "adsb_fix.h"

namespace adsbk {

// What the entry points accept (a NaN fails every comparison)
inline bool clock_cfg_ok(const adsb_clock_cfg &c, uint32_t n_receivers)
{
    if (c.time_source > ADSB_MLAT_TIME_TICKS || (c.flags & ~ADSB_CLOCK_DRIFT) != 0 || c.reference >= n_receivers)
        return false;
    const bool ticks = c.time_source == ADSB_MLAT_TIME_TICKS;
    const bool spt = ticks ? c.seconds_per_tick >= 0.0 : c.seconds_per_tick > 0.0;
    const bool sptime = ticks ? c.seconds_per_time > 0.0 : c.seconds_per_time >= 0.0;
    return spt && c.seconds_per_tick <= 1.0 && sptime && c.seconds_per_time <= 1.0 && c.max_residual_s >= 0.0 &&
           c.max_residual_s <= 1e6 && c.max_range_nm >= 0.0 && c.max_range_nm <= 180.0;
}

inline ClockParams clock_params_of(const adsb_clock_cfg &c)
{
    adsb_mlat_cfg m{};
    m.time_source = c.time_source;
    m.seconds_per_tick = c.seconds_per_tick;
    ClockParams p;
    p.time_source = c.time_source;
    p.flags = c.flags;
    p.reference = c.reference;
    p.min_rows = c.min_rows ? c.min_rows : 1u;
    p.seconds_per_tick = mlat_params_of(m).seconds_per_tick; // multilaterate's default
    p.seconds_per_time = c.seconds_per_time != 0.0 ? c.seconds_per_time : p.seconds_per_tick;
    p.max_residual_s = c.max_residual_s;
    p.max_range_nm = c.max_range_nm != 0.0 ? c.max_range_nm : 180.0;
    return p;
}

// A message's own time
ADSB_MLAT_HD inline double clock_tau(uint64_t msg_time, uint64_t first_msg_time, double seconds_per_time)
{
#pragma clang fp contract(off)
    return (double)(int64_t)(msg_time - first_msg_time) * seconds_per_time;
}

// geodetic (degrees, metres) -> ECEF: mlat_station_of's formula, which is host only, in the same order of operations.
ADSB_MLAT_HD inline void clock_ecef(double latitude, double longitude, double height_m, double *p)
{
#pragma clang fp contract(off)
    const double phi = latitude * kMlatRad, lam = longitude * kMlatRad;
    const double sp = sin(phi), cp = cos(phi);
    const double n = kMlatA / sqrt(1.0 - kMlatE2 * (sp * sp));
    p[0] = (n + height_m) * cp * cos(lam);
    p[1] = (n + height_m) * cp * sin(lam);
    p[2] = (n * (1.0 - kMlatE2) + height_m) * sp;
}

// Where an eligible message was sent from, decoded against the receiver of its first used reception.  false: no rows.
// (The counts -- at most ADSB_MLAT_MAX_RECEPTIONS receptions, two used -- are the caller's.)
ADSB_MLAT_HD inline bool clock_position(const ClockParams &c, const ClockStation &first, const uint8_t *bytes, double *p)
{
#pragma clang fp contract(off)
    double alt_m = 0.0;
    if (!mlat_altitude_of(bytes, alt_m)) return false; // the Q bit and a non-zero code
    adsb_site site;
    site.latitude = first.latitude;
    site.longitude = first.longitude;
    site.max_range_nm = c.max_range_nm;
    adsb_frame_fix f;
    FixRem r;
    fix_decode(site, bytes, f, r);
    const uint32_t want = ADSB_FIX_VALID | ADSB_FIX_ALT;
    if ((f.flags & (want | ADSB_FIX_SURFACE)) != want) return false;
    clock_ecef(f.latitude, f.longitude, (double)r.altitude * 0.3048, p);
    return true;
}

// A row's y: i the first used reception's station, j this one's.
ADSB_MLAT_HD inline double clock_row_y(const ClockParams &c, int64_t dticks, const MlatStation &si, const MlatStation &sj,
                                       const double *p)
{
#pragma clang fp contract(off)
    const double ri = mlat_dist(p, si.x, si.y, si.z), rj = mlat_dist(p, sj.x, sj.y, sj.z);
    return (double)dticks * c.seconds_per_tick - (sj.clock - si.clock) - (rj - ri) / kMlatC;
}

// The pair key of a row (i != j; a row with i == j cannot be: one used reception per receiver) and its oriented y'.
ADSB_MLAT_HD inline uint32_t clock_key(uint32_t i, uint32_t j, double y, double &yp)
{
    const uint32_t lo = i < j ? i : j, hi = i < j ? j : i;
    yp = j == hi ? y : -y;
    return lo << 8 | hi;
}

ADSB_MLAT_HD inline uint32_t clock_pair_at(uint32_t lo, uint32_t hi) // where the pair's sums lie: [256 x 256]
{
    return lo << 8 | hi;
}

// One partial sum of a pair.
struct ClockPart {
    double v[5]; // tau, tau^2, y', tau y', y'^2
};

ADSB_MLAT_HD inline void clock_part_zero(ClockPart &s)
{
    for (int k = 0; k < 5; ++k) s.v[k] = 0.0;
}

ADSB_MLAT_HD inline void clock_part_add(ClockPart &s, double tau, double yp)
{
#pragma clang fp contract(off)
    s.v[0] += tau;
    s.v[1] += tau * tau;
    s.v[2] += yp;
    s.v[3] += tau * yp;
    s.v[4] += yp * yp;
}

// The butterfly over 64 partial values held in one array (the mirror; the device's lanes do the same with shuffles).
inline double clock_fold64(const double *partial)
{
#pragma clang fp contract(off)
    double v[kClockPartials], w[kClockPartials];
    for (uint32_t l = 0; l < kClockPartials; ++l) v[l] = partial[l];
    for (uint32_t m = kClockPartials / 2; m; m >>= 1) {
        for (uint32_t l = 0; l < kClockPartials; ++l) w[l] = v[l] + v[l ^ m];
        for (uint32_t l = 0; l < kClockPartials; ++l) v[l] = w[l];
    }
    return v[0];
}

ADSB_MLAT_HD inline const ClockPair &clock_pair_of(const ClockPair *pairs, uint32_t u, uint32_t v)
{
    return pairs[u < v ? clock_pair_at(u, v) : clock_pair_at(v, u)];
}

ADSB_MLAT_HD inline bool clock_edge(const ClockParams &c, const ClockPair *pairs, uint32_t u, uint32_t v)
{
    return u != v && clock_pair_of(pairs, u, v).n >= (uint64_t)c.min_rows;
}

// The sum a pair gives to the entry between an unknown of kind ku and one of kind kv (0: a, 1: b)
ADSB_MLAT_HD inline double clock_pair_term(const ClockPair &q, uint32_t ku, uint32_t kv)
{
    return ku + kv == 0 ? (double)q.n : ku + kv == 1 ? q.st : q.stt;
}

// Entry of the normal matrix between unknown (receiver ru, kind ku) and unknown (rv, kv).  R: the receivers.
ADSB_MLAT_HD inline double clock_normal_entry(const ClockParams &c, const ClockPair *pairs, uint32_t R, uint32_t ru,
                                              uint32_t ku, uint32_t rv, uint32_t kv)
{
#pragma clang fp contract(off)
    if (ru != rv) return clock_edge(c, pairs, ru, rv) ? -clock_pair_term(clock_pair_of(pairs, ru, rv), ku, kv) : 0.0;
    double v = 0.0;
    for (uint32_t w = 0; w < R; ++w)
        if (clock_edge(c, pairs, ru, w)) v += clock_pair_term(clock_pair_of(pairs, ru, w), ku, kv);
    return v;
}

// Entry of the right-hand side for unknown (ru, ku)
ADSB_MLAT_HD inline double clock_rhs_entry(const ClockParams &c, const ClockPair *pairs, uint32_t R, uint32_t ru,
                                           uint32_t ku)
{
#pragma clang fp contract(off)
    double v = 0.0;
    for (uint32_t w = 0; w < R; ++w) {
        if (!clock_edge(c, pairs, ru, w)) continue;
        const ClockPair &q = clock_pair_of(pairs, ru, w);
        const double t = ku ? q.sty : q.sy;
        if (w < ru) v += t; // ru is the pair's hi
        else v -= t;
    }
    return v;
}

// Entry (i, j), j <= i, of the left-looking factorisation in place: m holds A's lower triangle (row-major, n x n) with
// columns < j already L, d the pivots so far.  For i == j the result is the pivot, else the entry before division.
ADSB_MLAT_HD inline double clock_ldl_entry(const double *m, const double *d, uint32_t n, uint32_t i, uint32_t j)
{
#pragma clang fp contract(off)
    double v = m[(size_t)i * n + j];
    for (uint32_t k = 0; k < j; ++k) v -= (m[(size_t)i * n + k] * d[k]) * m[(size_t)j * n + k];
    return v;
}

ADSB_MLAT_HD inline bool clock_pivot_ok(double pivot, double diagonal)
{
#pragma clang fp contract(off)
    return pivot > kMlatPivot * diagonal;
}

// A row's residual under a solution; lo, hi: the pair's receivers' solutions.
ADSB_MLAT_HD inline double clock_residual(double yp, double tau, const ClockSol &lo, const ClockSol &hi)
{
#pragma clang fp contract(off)
    return yp - ((hi.a + hi.b * tau) - (lo.a + lo.b * tau));
}

// The squared residuals of a pair's rows, from its sums.
ADSB_MLAT_HD inline double clock_pair_ssr(const ClockPair &q, const ClockSol &lo, const ClockSol &hi)
{
#pragma clang fp contract(off)
    const double da = hi.a - lo.a, db = hi.b - lo.b;
    return q.syy - 2.0 * da * q.sy - 2.0 * db * q.sty + da * da * (double)q.n + 2.0 * da * db * q.st + db * db * q.stt;
}

// Receiver u's record.  first: the pairs' sums before dropping (the same array when there was one pass).
ADSB_MLAT_HD inline adsb_clock clock_record(const ClockParams &c, const ClockPair *pairs, const ClockPair *first,
                                            uint32_t R, uint32_t u, const ClockSol *sol, double prior, bool reached,
                                            bool drift)
{
#pragma clang fp contract(off)
    adsb_clock o;
    o.offset_s = prior + sol[u].a;
    o.fine_offset_s = sol[u].a;
    o.drift = sol[u].b;
    uint64_t rows = 0, before = 0;
    uint32_t partners = 0;
    double ssr = 0.0;
    for (uint32_t w = 0; w < R; ++w) {
        if (w == u) continue;
        const ClockPair &q = clock_pair_of(pairs, u, w);
        before += clock_pair_of(first, u, w).n;
        if (q.n == 0) continue;
        rows += q.n;
        if (clock_edge(c, pairs, u, w)) ++partners;
        ssr += u < w ? clock_pair_ssr(q, sol[u], sol[w]) : clock_pair_ssr(q, sol[w], sol[u]);
    }
    o.residual_rms_s = rows ? (float)sqrt((ssr > 0.0 ? ssr : 0.0) / (double)rows) : 0.0f;
    o.n_rows = (uint32_t)rows;
    o.n_dropped = (uint32_t)(before - rows);
    o.n_partners = partners;
    o.flags = (u == c.reference ? ADSB_CLOCK_REFERENCE : 0u) | (reached ? ADSB_CLOCK_REACHED : 0u) |
              (reached && drift && u != c.reference ? ADSB_CLOCK_HAS_DRIFT : 0u);
    for (int k = 0; k < 5; ++k) o.reserved[k] = 0;
    return o;
}

// A reception's corrected time: d its raw time against the list's first, in ticks.
ADSB_MLAT_HD inline uint64_t clock_apply_time(int64_t d, double offset_s, double drift, double tau, double spt)
{
#pragma clang fp contract(off)
    const long long shift = llrint(256.0 * (offset_s + drift * tau) / spt);
    return 256ull * (uint64_t)d - (uint64_t)shift;
}

// What a message gives the header
constexpr uint8_t kClockMsgEligible = 1, kClockMsgBad = 2;

} // namespace adsbk

#endif
