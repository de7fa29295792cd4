// adsb_track_es.h -- a table's extended squitter step (include/adsb_hip.h, "Extended squitter status per aircraft"):
// which frames count, the version and NIC supplements a position message is resolved against, the per-frame output,
// what ONE counted frame contributes to its aircraft's es record, the empty record, and the combine of a record with a
// later one.  One text for the device (adsb_track.hip: one thread per frame resolves and writes the scan's operand, one
// thread per segment tail builds the segment's part and merges it) and the CPU mirror (host/adsb_track_es.cpp): every
// function here is __host__ __device__ under hipcc and plain inline C++ otherwise.  Integers, one f64 subtraction and
// two comparisons for an age, and times that are copied: nothing can differ between the two sides.  NIC and Rc come
// from adsb_es.h's es_integrity, which is called here and not restated.
#ifndef ADSB_TRACK_ES_H
#define ADSB_TRACK_ES_H

#include "adsb_es.h"

namespace adsbk {

static_assert(sizeof(adsb_aircraft_es) == 256 && sizeof(adsb_frame_integrity) == 8 && sizeof(adsb_es_track_cfg) == 16,
              "es track records");

// The groups of an es record that "the later frame wins" applies to, each on its own: the five blocks in the
// record's order, then version, NIC supplement A, NIC supplement C, position, category, NACv
constexpr uint32_t kEsTrackOpAir = 0, kEsTrackOpSurface = 1, kEsTrackTargetState = 2, kEsTrackEmergency = 3,
                   kEsTrackAcasRa = 4, kEsTrackVersion = 5, kEsTrackNicA = 6, kEsTrackNicC = 7, kEsTrackPosition = 8,
                   kEsTrackCategory = 9, kEsTrackNacV = 10, kEsTrackGroups = 11;

// counted by its record (its key and its point are the caller's to test)
ADSB_WIRE_HD inline bool es_track_counted(const adsb_es_rec &r)
{
    return r.state != ADSB_ES_NOT_ES && r.state != ADSB_ES_FOREIGN;
}

// bit g: a counted frame with this record writes group g
ADSB_WIRE_HD inline uint32_t es_track_writes(const adsb_es_rec &r)
{
    uint32_t m = 0;
    if (r.state == ADSB_ES_OPERATIONAL && r.subtype == 0u) m |= 1u << kEsTrackOpAir;
    if (r.state == ADSB_ES_OPERATIONAL && r.subtype == 1u) m |= 1u << kEsTrackOpSurface;
    if (r.state == ADSB_ES_TARGET_STATE) m |= 1u << kEsTrackTargetState;
    if (r.state == ADSB_ES_EMERGENCY) m |= 1u << kEsTrackEmergency;
    if (r.state == ADSB_ES_ACAS_RA) m |= 1u << kEsTrackAcasRa;
    if (r.present & ADSB_ES_HAS_VERSION) m |= 1u << kEsTrackVersion;
    if (r.present & ADSB_ES_HAS_NIC_A) m |= 1u << kEsTrackNicA;
    if (r.present & ADSB_ES_HAS_NIC_C) m |= 1u << kEsTrackNicC;
    if (r.state == ADSB_ES_POSITION) m |= 1u << kEsTrackPosition;
    if (r.state == ADSB_ES_CATEGORY) m |= 1u << kEsTrackCategory;
    if (r.present & ADSB_ES_HAS_NAC_V) m |= 1u << kEsTrackNacV;
    return m;
}

// What a frame is resolved against: the aircraft's newest earlier version, supplement A and supplement C; a time of NaN:
// the aircraft has none
struct EsKnown {
    double version_time, a_time, c_time;
    uint32_t version, a, c;
};

ADSB_WIRE_HD inline EsKnown es_known_none()
{
    EsKnown k;
    k.version_time = k.a_time = k.c_time = __builtin_nan("");
    k.version = k.a = k.c = 0u;
    return k;
}

ADSB_WIRE_HD inline EsKnown es_known_of_record(const adsb_aircraft_es &a)
{
    EsKnown k;
    k.version_time = a.version_time;
    k.a_time = a.nic_a_time;
    k.c_time = a.nic_c_time;
    k.version = a.version;
    k.a = a.nic_a;
    k.c = a.nic_c;
    return k;
}

// usable iff 0 <= t - time <= max_age_s: one f64 subtraction; NaN anywhere is not usable
ADSB_WIRE_HD inline bool es_track_usable(double time, double t, double max_age_s)
{
    const double age = t - time;
    return age >= 0.0 && age <= max_age_s;
}

// The per-frame output of a frame with record r heard at t, of an aircraft that knows k, whose key and point let it
// count.  All zero for a record that does not count.
ADSB_WIRE_HD inline adsb_frame_integrity es_track_resolve(const adsb_es_rec &r, double t, const EsKnown &k, double max_age_s)
{
    adsb_frame_integrity o;
    o.rc_dm = 0u;
    o.nic = o.version = o.supp = o.flags = 0u;
    if (!es_track_counted(r)) return o;
    const bool versioned = k.version_time == k.version_time;
    o.flags = ADSB_TRACK_ES_COUNTED;
    o.version = versioned ? (uint8_t)k.version : (uint8_t)ADSB_ES_VERSION_UNKNOWN;
    if (r.state != ADSB_ES_POSITION) return o;
    uint32_t flags = ADSB_TRACK_ES_COUNTED | ADSB_TRACK_ES_POSITION | (versioned ? ADSB_TRACK_ES_VERSIONED : 0u), supp = 0u;
    if (k.a_time == k.a_time) {
        if (es_track_usable(k.a_time, t, max_age_s)) supp |= k.a & 1u;
        else flags |= ADSB_TRACK_ES_STALE_A;
    }
    if (r.present & ADSB_ES_HAS_NIC_B) supp |= (r.nic_b & 1u) << 1;
    if (k.c_time == k.c_time) {
        if (es_track_usable(k.c_time, t, max_age_s)) supp |= (k.c & 1u) << 2;
        else flags |= ADSB_TRACK_ES_STALE_C;
    }
    const EsIntegrity g = es_integrity(r.type_code, o.version, supp);
    o.rc_dm = g.rc_dm;
    o.nic = (uint8_t)g.nic;
    o.supp = (uint8_t)supp;
    o.flags = (uint8_t)flags;
    return o;
}

// The 256 bytes of an es record as words, for stores and moves
struct EsWords {
    uint64_t w[32];
};

// The empty record: every time NaN, all else zero
ADSB_WIRE_HD inline adsb_aircraft_es es_track_empty_record()
{
    adsb_aircraft_es a;
    __builtin_memset(&a, 0, sizeof(a));
    const double none = __builtin_nan("");
    a.time[0] = a.time[1] = a.time[2] = a.time[3] = a.time[4] = none;
    a.version_time = a.nic_a_time = a.nic_c_time = a.position_time = none;
    return a;
}

ADSB_WIRE_HD inline EsWords es_track_empty()
{
    const adsb_aircraft_es a = es_track_empty_record();
    EsWords o;
    __builtin_memcpy(&o, &a, sizeof(o));
    return o;
}

// to = from, as eight 32-bit words (the record's alignment), written out: a block moves as words, like the record
// itself, and stays in registers on the device (a struct copy of byte members does not)
typedef uint32_t __attribute__((may_alias)) EsRecWord;
ADSB_WIRE_HD inline void es_rec_copy(adsb_es_rec &to, const adsb_es_rec &from)
{
    const EsRecWord *s = (const EsRecWord *)&from;
    EsRecWord *d = (EsRecWord *)&to;
    const uint32_t w0 = s[0], w1 = s[1], w2 = s[2], w3 = s[3], w4 = s[4], w5 = s[5], w6 = s[6], w7 = s[7];
    d[0] = w0, d[1] = w1, d[2] = w2, d[3] = w3, d[4] = w4, d[5] = w5, d[6] = w6, d[7] = w7;
}
static_assert(sizeof(adsb_es_rec) == 32 && alignof(adsb_es_rec) == 4, "es_rec_copy");

// Group g (a constant where it is called) of `a` as a counted frame with record r and per-frame output f, heard at t,
// writes it
ADSB_WIRE_HD inline void es_track_set(adsb_aircraft_es &a, uint32_t g, const adsb_es_rec &r, const adsb_frame_integrity &f,
                                      double t)
{
    switch (g) {
    case kEsTrackOpAir: es_rec_copy(a.operational_airborne, r); a.time[0] = t; break;
    case kEsTrackOpSurface: es_rec_copy(a.operational_surface, r); a.time[1] = t; break;
    case kEsTrackTargetState: es_rec_copy(a.target_state, r); a.time[2] = t; break;
    case kEsTrackEmergency: es_rec_copy(a.emergency, r); a.time[3] = t; break;
    case kEsTrackAcasRa: es_rec_copy(a.acas_ra, r); a.time[4] = t; break;
    case kEsTrackVersion: a.version = r.version; a.version_time = t; break;
    case kEsTrackNicA: a.nic_a = r.nic_a; a.nic_a_time = t; break;
    case kEsTrackNicC: a.nic_c = r.nic_c; a.nic_c_time = t; break;
    case kEsTrackPosition:
        a.rc_dm = f.rc_dm;
        a.nic = f.nic;
        a.position_tc = r.type_code;
        a.nic_b = (r.present & ADSB_ES_HAS_NIC_B) ? r.nic_b : (uint8_t)0;
        a.position_supp = (uint8_t)(f.supp | (f.flags & (ADSB_TRACK_ES_VERSIONED | ADSB_TRACK_ES_STALE_A | ADSB_TRACK_ES_STALE_C)) << 1);
        a.position_time = t;
        break;
    case kEsTrackCategory: a.category = r.category; break;
    case kEsTrackNacV:
        a.nac_v = r.nac_v;
        a.velocity_flags = r.state == ADSB_ES_VELOCITY ? (uint8_t)(r.flags & 0xFFu) : (uint8_t)0;
        a.has = r.state == ADSB_ES_VELOCITY ? (uint8_t)3 : (uint8_t)1;
        break;
    default: break;
    }
}

// The record of an aircraft whose only counted frame since admission has record r and per-frame output f; the empty
// record if f is not COUNTED
ADSB_WIRE_HD inline adsb_aircraft_es es_track_one(const adsb_es_rec &r, const adsb_frame_integrity &f, double t)
{
    adsb_aircraft_es a = es_track_empty_record();
    if (!(f.flags & ADSB_TRACK_ES_COUNTED)) return a;
    const uint32_t m = es_track_writes(r);
    a.n_es = 1u;
    a.n_position = (m >> kEsTrackPosition) & 1u;
    if (m & (1u << kEsTrackOpAir)) es_track_set(a, kEsTrackOpAir, r, f, t);
    if (m & (1u << kEsTrackOpSurface)) es_track_set(a, kEsTrackOpSurface, r, f, t);
    if (m & (1u << kEsTrackTargetState)) es_track_set(a, kEsTrackTargetState, r, f, t);
    if (m & (1u << kEsTrackEmergency)) es_track_set(a, kEsTrackEmergency, r, f, t);
    if (m & (1u << kEsTrackAcasRa)) es_track_set(a, kEsTrackAcasRa, r, f, t);
    if (m & (1u << kEsTrackVersion)) es_track_set(a, kEsTrackVersion, r, f, t);
    if (m & (1u << kEsTrackNicA)) es_track_set(a, kEsTrackNicA, r, f, t);
    if (m & (1u << kEsTrackNicC)) es_track_set(a, kEsTrackNicC, r, f, t);
    if (m & (1u << kEsTrackPosition)) es_track_set(a, kEsTrackPosition, r, f, t);
    if (m & (1u << kEsTrackCategory)) es_track_set(a, kEsTrackCategory, r, f, t);
    if (m & (1u << kEsTrackNacV)) es_track_set(a, kEsTrackNacV, r, f, t);
    return a;
}

ADSB_WIRE_HD inline uint32_t es_track_sat_add(uint32_t a, uint32_t b)
{
    const uint32_t c = a + b;
    return c < a ? ~0u : c;
}

// `into` followed by `later`, a record of the frames that come after into's.  A part holds a block, a version, a
// supplement or a position iff that time is no NaN, a category iff it is not 0, a NACv iff has is not 0.  Associative;
// the empty record is its identity.
ADSB_WIRE_HD inline void es_track_merge(adsb_aircraft_es &into, const adsb_aircraft_es &later)
{
    if (later.time[0] == later.time[0]) { es_rec_copy(into.operational_airborne, later.operational_airborne); into.time[0] = later.time[0]; }
    if (later.time[1] == later.time[1]) { es_rec_copy(into.operational_surface, later.operational_surface); into.time[1] = later.time[1]; }
    if (later.time[2] == later.time[2]) { es_rec_copy(into.target_state, later.target_state); into.time[2] = later.time[2]; }
    if (later.time[3] == later.time[3]) { es_rec_copy(into.emergency, later.emergency); into.time[3] = later.time[3]; }
    if (later.time[4] == later.time[4]) { es_rec_copy(into.acas_ra, later.acas_ra); into.time[4] = later.time[4]; }
    if (later.version_time == later.version_time) {
        into.version = later.version;
        into.version_time = later.version_time;
    }
    if (later.nic_a_time == later.nic_a_time) {
        into.nic_a = later.nic_a;
        into.nic_a_time = later.nic_a_time;
    }
    if (later.nic_c_time == later.nic_c_time) {
        into.nic_c = later.nic_c;
        into.nic_c_time = later.nic_c_time;
    }
    if (later.position_time == later.position_time) {
        into.rc_dm = later.rc_dm;
        into.nic = later.nic;
        into.position_tc = later.position_tc;
        into.nic_b = later.nic_b;
        into.position_supp = later.position_supp;
        into.position_time = later.position_time;
    }
    if (later.category != 0u) into.category = later.category;
    if (later.has != 0u) {
        into.nac_v = later.nac_v;
        into.velocity_flags = later.velocity_flags;
        into.has = later.has;
    }
    into.n_es = es_track_sat_add(into.n_es, later.n_es);
    into.n_position = es_track_sat_add(into.n_position, later.n_position);
}

} // namespace adsbk
#endif
