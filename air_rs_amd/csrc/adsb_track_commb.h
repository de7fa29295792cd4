// adsb_track_commb.h -- a table's Comm-B step (include/adsb_hip.h, "Comm-B registers per aircraft"): the reference an
// ambiguous {5,0; 6,0} reply is settled against, sector16, the checks and the decision, what ONE counted frame
// contributes to its aircraft's commb record, the empty record, and the combine of a record with a later one.  One text
// for the device (adsb_track.hip: one thread per frame settles and writes the scan's operand, one thread per segment
// tail builds the segment's part and merges it) and the CPU mirror (host/adsb_track_commb.cpp): every function here is
// __host__ __device__ under hipcc and plain inline C++ otherwise.  Integers, one f64 subtraction and two comparisons
// for the age, and times that are copied: nothing can differ between the two sides.  The registers' values come from
// adsb_commb.h's commb_decode, which is called here and not restated.
#ifndef ADSB_TRACK_COMMB_H
#define ADSB_TRACK_COMMB_H

#include "adsb_commb.h"

namespace adsbk {

static_assert(sizeof(adsb_aircraft_commb) == 128 && sizeof(adsb_commb_block) == 32 && sizeof(adsb_commb_settle_cfg) == 16,
              "commb records");

// The exact fields of an airborne-velocity message the rule reads; subtype 0: none
struct CommbRef {
    double time;
    int32_t ew, ns, vr; // ST 1-2 with SPEED; with VRATE
    int32_t speed;      // ST 3-4 with SPEED: the airspeed
    int32_t h10;        // ST 3-4 with DIRECTION: the 10-bit heading
    uint32_t subtype, flags, tas;
};

ADSB_WIRE_HD inline CommbRef commb_ref_none()
{
    CommbRef r;
    r.time = __builtin_nan("");
    r.ew = r.ns = r.vr = r.speed = r.h10 = 0;
    r.subtype = r.flags = r.tas = 0;
    return r;
}

// From the held adsb_velocity.  ST 3-4: speed_kt is an integer value and direction_deg x 128 / 45 an exact integer;
// direction_deg and speed_kt of ST 1-2 are never read.
ADSB_WIRE_HD inline CommbRef commb_ref_of_velocity(const adsb_velocity &v)
{
    CommbRef r = commb_ref_none();
    if (v.subtype < 1 || v.subtype > 4) return r;
    r.time = v.time;
    r.subtype = v.subtype;
    r.flags = v.flags;
    r.vr = v.vertical_rate_fpm;
    if (v.subtype <= 2) {
        r.ew = v.v_ew_kt;
        r.ns = v.v_ns_kt;
    } else {
        r.speed = (int32_t)v.speed_kt;
        r.h10 = (int32_t)((double)v.direction_deg * 128.0 / 45.0);
        r.tas = v.airspeed_tas;
    }
    return r;
}

// From the 14 bytes of a DF17/18 TC 19 frame, by the header's airborne-velocity rules in integers; subtype 0 for ST 0
// and 5-7.  The same fields commb_ref_of_velocity gives for the adsb_velocity the table decodes from these bytes.
ADSB_WIRE_HD inline CommbRef commb_ref_of_frame(const ModesBytes &b, double time)
{
    CommbRef r = commb_ref_none();
    const uint64_t me = (b.w0 & 0xFFFFFFFFull) << 24 | b.w1 >> 40; // ME bit 0 in bit 55
    const uint32_t st = (uint32_t)(me >> 48) & 7u;
    if (st < 1 || st > 4) return r;
    const int32_t k = (st == 2 || st == 4) ? 4 : 1;
    r.time = time;
    r.subtype = st;
    const uint32_t f13 = (uint32_t)(me >> 42) & 1u, f14 = (uint32_t)(me >> 32) & 1023u, f24 = (uint32_t)(me >> 31) & 1u,
                   f25 = (uint32_t)(me >> 21) & 1023u;
    if (st <= 2) {
        if (f14 != 0 && f25 != 0) {
            r.ew = (f13 ? -1 : 1) * (int32_t)(f14 - 1u) * k;
            r.ns = (f24 ? -1 : 1) * (int32_t)(f25 - 1u) * k;
            r.flags = ADSB_VELOCITY_SPEED | ((r.ew != 0 || r.ns != 0) ? ADSB_VELOCITY_DIRECTION : 0u);
        }
    } else {
        if (f13) {
            r.h10 = (int32_t)f14;
            r.flags = ADSB_VELOCITY_DIRECTION;
        }
        if (f25 != 0) {
            r.speed = (int32_t)(f25 - 1u) * k;
            r.tas = f24;
            r.flags |= ADSB_VELOCITY_SPEED;
        }
    }
    const uint32_t vr = (uint32_t)(me >> 10) & 511u;
    if (vr != 0) {
        r.vr = (((me >> 19) & 1u) ? -1 : 1) * (int32_t)(vr - 1u) * 64;
        r.flags |= ADSB_VELOCITY_VRATE;
    }
    return r;
}

// usable iff 0 <= t_frame - R.time <= max_age_s: one f64 subtraction; NaN anywhere is not usable
ADSB_WIRE_HD inline bool commb_ref_usable(const CommbRef &r, double t_frame, double max_age_s)
{
    if (r.subtype == 0) return false;
    const double age = t_frame - r.time;
    return age >= 0.0 && age <= max_age_s;
}

ADSB_WIRE_HD inline uint32_t commb_sector16(int32_t ew, int32_t ns)
{
    const int32_t a = ew < 0 ? -ew : ew, b = ns < 0 ? -ns : ns;
    uint32_t k;
    if (985 * a < 408 * b) k = 0;
    else if (a < b) k = 1;
    else if (408 * a < 985 * b) k = 2;
    else k = 3;
    if (ew >= 0 && ns > 0) return k;
    if (ew > 0 && ns <= 0) return 7u - k;
    if (ew <= 0 && ns < 0) return 8u + k;
    return 15u - k;
}

ADSB_WIRE_HD inline uint32_t commb_circular(uint32_t x, uint32_t y, uint32_t modulus) // modulus a power of two
{
    const uint32_t d = (x - y) & (modulus - 1u);
    return d < modulus - d ? d : modulus - d;
}

ADSB_WIRE_HD inline bool commb_within(int32_t x, int32_t y, uint32_t limit)
{
    const int64_t d = (int64_t)x - (int64_t)y;
    return (uint64_t)(d < 0 ? -d : d) <= (uint64_t)limit;
}

// applied and failed checks of one reading
struct CommbChecks {
    uint32_t applied, failed;
    ADSB_WIRE_HD void check(bool pass)
    {
        ++applied;
        if (!pass) ++failed;
    }
    ADSB_WIRE_HD bool supported() const { return applied != 0 && failed == 0; }
    ADSB_WIRE_HD bool contradicted() const { return failed != 0; }
};

// r: the ONE record of the reading as 5,0
ADSB_WIRE_HD inline CommbChecks commb_checks_50(const adsb_commb_rec &r, const CommbRef &v, const adsb_commb_settle_cfg &cfg)
{
    CommbChecks c{0, 0};
    const bool ground = v.subtype <= 2 && (v.flags & ADSB_VELOCITY_SPEED);
    const int64_t s2 = (int64_t)v.ew * v.ew + (int64_t)v.ns * v.ns; // < 2^26
    if ((r.status & 4u) && ground) {
        const uint64_t g = (uint64_t)(uint32_t)r.value[2], S = cfg.max_speed_diff_kt;
        const uint64_t lo = g > S ? g - S : 0u;
        uint64_t hi = g + S;
        if (hi > 0xFFFFFu) hi = 0xFFFFFu; // s2 is below its square anyway
        c.check(lo * lo <= (uint64_t)s2 && (uint64_t)s2 <= hi * hi);
    }
    if ((r.status & 2u) && ground && s2 > 0)
        c.check(commb_circular((uint32_t)r.value[1] >> 7, commb_sector16(v.ew, v.ns), 16u) <= 1u);
    if ((r.status & 16u) && v.subtype >= 3 && (v.flags & ADSB_VELOCITY_SPEED) && v.tas == 1u)
        c.check(commb_within(r.value[4], v.speed, cfg.max_speed_diff_kt));
    return c;
}

// r: the ONE record of the reading as 6,0
ADSB_WIRE_HD inline CommbChecks commb_checks_60(const adsb_commb_rec &r, const CommbRef &v, const adsb_commb_settle_cfg &cfg)
{
    CommbChecks c{0, 0};
    const bool ground = v.subtype <= 2 && (v.flags & ADSB_VELOCITY_SPEED);
    if ((r.status & 1u) && ground && (v.ew != 0 || v.ns != 0))
        c.check(commb_circular((uint32_t)r.value[0] >> 7, commb_sector16(v.ew, v.ns), 16u) <= 2u);
    if ((r.status & 1u) && v.subtype >= 3 && (v.flags & ADSB_VELOCITY_DIRECTION))
        c.check(commb_circular((uint32_t)r.value[0], 2u * (uint32_t)v.h10, 2048u) <= 128u);
    if ((r.status & 2u) && v.subtype >= 3 && (v.flags & ADSB_VELOCITY_SPEED) && v.tas == 0u)
        c.check(commb_within(r.value[1], v.speed, cfg.max_speed_diff_kt));
    if ((r.status & 8u) && (v.flags & ADSB_VELOCITY_VRATE)) c.check(commb_within(r.value[3], v.vr, cfg.max_vrate_diff_fpm));
    if ((r.status & 16u) && (v.flags & ADSB_VELOCITY_VRATE)) c.check(commb_within(r.value[4], v.vr, cfg.max_vrate_diff_fpm));
    return c;
}

ADSB_WIRE_HD inline bool commb_can_settle(const adsb_commb_rec &r)
{
    return r.state == ADSB_COMMB_AMBIGUOUS && r.candidates == (ADSB_COMMB_C50 | ADSB_COMMB_C60);
}

// The per-frame output of a COUNTED frame with bytes b and stateless record r, heard at t_frame, against the reference v
// (subtype 0: none): r itself, or the SETTLED record
ADSB_WIRE_HD inline adsb_commb_rec commb_settle(const ModesBytes &b, const adsb_commb_rec &r, const CommbRef &v,
                                                double t_frame, const adsb_commb_settle_cfg &cfg)
{
    if (!commb_can_settle(r) || !commb_ref_usable(v, t_frame, cfg.max_age_s)) return r;
    const CommbMb m = commb_mb(b);
    adsb_commb_rec r5 = r, r6 = r;
    commb_decode(m, ADSB_COMMB_C50, r5);
    commb_decode(m, ADSB_COMMB_C60, r6);
    const CommbChecks c5 = commb_checks_50(r5, v, cfg), c6 = commb_checks_60(r6, v, cfg);
    if (c5.supported() && c6.contradicted()) {
        r5.state = ADSB_COMMB_SETTLED;
        return r5;
    }
    if (c6.supported() && c5.contradicted()) {
        r6.state = ADSB_COMMB_SETTLED;
        return r6;
    }
    return r;
}

// What a counted frame's per-frame output writes: one of the five "newest" sorts, or none
constexpr uint32_t kCommbSort40 = 0, kCommbSort50 = 1, kCommbSort60 = 2, kCommbSort17 = 3, kCommbSort30 = 4,
                   kCommbSortNone = 5;
ADSB_WIRE_HD inline uint32_t commb_sort_of(const adsb_commb_rec &r)
{
    if (r.state != ADSB_COMMB_ONE && r.state != ADSB_COMMB_SETTLED) return kCommbSortNone;
    if (r.bds == 0x40u) return kCommbSort40;
    if (r.bds == 0x50u) return kCommbSort50;
    if (r.bds == 0x60u) return kCommbSort60;
    if (r.state == ADSB_COMMB_ONE && r.bds == 0x17u && r.word != 0u) return kCommbSort17;
    if (r.state == ADSB_COMMB_ONE && r.bds == 0x30u) return kCommbSort30;
    return kCommbSortNone;
}

// The 128 bytes of a commb record as words, for stores and moves
struct CommbWords {
    uint64_t w[16];
};

ADSB_WIRE_HD inline adsb_commb_block commb_block_empty()
{
    adsb_commb_block k;
    __builtin_memset(&k, 0, sizeof(k));
    k.time = __builtin_nan("");
    return k;
}

// The empty record: every time NaN, all else zero
ADSB_WIRE_HD inline adsb_aircraft_commb commb_empty_record()
{
    adsb_aircraft_commb a;
    __builtin_memset(&a, 0, sizeof(a));
    a.bds40 = a.bds50 = a.bds60 = commb_block_empty();
    a.ra_time = __builtin_nan("");
    return a;
}

ADSB_WIRE_HD inline CommbWords commb_empty()
{
    const adsb_aircraft_commb a = commb_empty_record();
    CommbWords o;
    __builtin_memcpy(&o, &a, sizeof(o));
    return o;
}

// the block a per-frame output of sort 4,0 / 5,0 / 6,0 makes
ADSB_WIRE_HD inline adsb_commb_block commb_block_of(const adsb_commb_rec &r, double time)
{
    adsb_commb_block k;
    k.time = time;
    for (int i = 0; i < 5; ++i) k.value[i] = r.value[i];
    k.status = r.status;
    k.settled = r.state == ADSB_COMMB_SETTLED ? 1u : 0u;
    return k;
}

// The counts of a run of counted frames
struct CommbCounts {
    uint32_t n_commb, n_settled, n_ambiguous, n_none;
};

// the counts of one per-frame output; all zero for NOT_COMMB (the frame is not counted)
ADSB_WIRE_HD inline CommbCounts commb_counts_of(const adsb_commb_rec &r)
{
    CommbCounts c;
    c.n_commb = r.state != ADSB_COMMB_NOT_COMMB ? 1u : 0u;
    c.n_settled = r.state == ADSB_COMMB_SETTLED ? 1u : 0u;
    c.n_ambiguous = r.state == ADSB_COMMB_AMBIGUOUS ? 1u : 0u;
    c.n_none = r.state == ADSB_COMMB_NONE ? 1u : 0u;
    return c;
}

// The record of a run of counted frames that starts from nothing: its counts, and the run's newest per-frame output of
// each sort (null: the run has none) with its time
ADSB_WIRE_HD inline adsb_aircraft_commb commb_part(const CommbCounts &c, const adsb_commb_rec *r40, double t40,
                                                   const adsb_commb_rec *r50, double t50, const adsb_commb_rec *r60,
                                                   double t60, const adsb_commb_rec *r17, const adsb_commb_rec *r30,
                                                   double t30)
{
    adsb_aircraft_commb a = commb_empty_record();
    a.n_commb = c.n_commb;
    a.n_settled = c.n_settled;
    a.n_ambiguous = c.n_ambiguous;
    a.n_none = c.n_none;
    if (r40) a.bds40 = commb_block_of(*r40, t40);
    if (r50) a.bds50 = commb_block_of(*r50, t50);
    if (r60) a.bds60 = commb_block_of(*r60, t60);
    if (r17) a.capability = r17->word;
    if (r30) {
        a.ra_word = r30->word;
        a.ra_time = t30;
    }
    return a;
}

ADSB_WIRE_HD inline uint32_t commb_sat_add(uint32_t a, uint32_t b)
{
    const uint32_t c = a + b;
    return c < a ? ~0u : c;
}

// `into` followed by `later`, a record of the frames that come after into's.  A part holds a block iff the block's time
// is no NaN, a capability iff it is not 0, a 3,0 word iff ra_time is no NaN.  Associative; the empty record is its
// identity.
ADSB_WIRE_HD inline void commb_merge(adsb_aircraft_commb &into, const adsb_aircraft_commb &later)
{
    if (later.bds40.time == later.bds40.time) into.bds40 = later.bds40;
    if (later.bds50.time == later.bds50.time) into.bds50 = later.bds50;
    if (later.bds60.time == later.bds60.time) into.bds60 = later.bds60;
    if (later.capability != 0u) into.capability = later.capability;
    if (later.ra_time == later.ra_time) {
        into.ra_word = later.ra_word;
        into.ra_time = later.ra_time;
    }
    into.n_commb = commb_sat_add(into.n_commb, later.n_commb);
    into.n_settled = commb_sat_add(into.n_settled, later.n_settled);
    into.n_ambiguous = commb_sat_add(into.n_ambiguous, later.n_ambiguous);
    into.n_none = commb_sat_add(into.n_none, later.n_none);
}

// The record of an aircraft whose only counted frame has this per-frame output
ADSB_WIRE_HD inline adsb_aircraft_commb commb_one(const adsb_commb_rec &r, double time)
{
    const uint32_t sort = commb_sort_of(r);
    return commb_part(commb_counts_of(r), sort == kCommbSort40 ? &r : nullptr, time, sort == kCommbSort50 ? &r : nullptr,
                      time, sort == kCommbSort60 ? &r : nullptr, time, sort == kCommbSort17 ? &r : nullptr,
                      sort == kCommbSort30 ? &r : nullptr, time);
}

} // namespace adsbk
#endif
