// adsb_track_modes.h -- what ONE frame's adsb_modes_rec contributes to its aircraft's modes record, the empty record,
// and the combine of a record with a later contribution: include/adsb_hip.h, "Mode S replies per aircraft".  One text
// for the device (adsb_track.hip: one thread per frame writes modes_what() into the scan, one thread per segment tail
// builds the segment's part with modes_part() and merges it with modes_merge()) and the CPU mirror
// (host/adsb_track_modes.cpp): every function here is __host__ __device__ under hipcc and plain inline C++ otherwise.
// Integers, moves and three times that are copied, never computed here: nothing can differ between the two sides.
#ifndef ADSB_TRACK_MODES_H
#define ADSB_TRACK_MODES_H

#include "adsb_fix.h"
#include "adsb_modes.h"

namespace adsbk {

static_assert(sizeof(adsb_aircraft_modes) == 64 && sizeof(adsb_modes_rec) == 32, "modes records");

// kModesNoAddress (adsb_modes.h, 1 << 24): the sort key of a frame that is not accepted, after every address
static_assert(kModesNoAddress == 1u << 24, "the 25-bit sort");

// What a counted frame writes, by its record alone
constexpr uint32_t kModesAlt = 0x1u, kModesSquawk = 0x2u, kModesCallsign = 0x4u, kModesStatus = 0x8u,
                   kModesGround = 0x10u, // the frame is a source of GROUND (set or clear), not the bit itself
    kModesSquitter = 0x20u, kModesReply = 0x40u, kModesAllcall = 0x80u, kModesSurveillance = 0x100u,
                   kModesAirAir = 0x200u;

ADSB_HD inline bool modes_accepted(const adsb_modes_rec &r)
{
    return r.kind == ADSB_MODES_SELF || r.kind == ADSB_MODES_KNOWN;
}

// DF17/18: the frame the main record reads as update does; every other DF is a frame of kind "other" there
ADSB_HD inline bool modes_squitter(uint32_t df) { return df == 17 || df == 18; }

// The per-frame contribution of an ACCEPTED frame: which fields it writes and which counts it adds to
ADSB_HD inline uint32_t modes_what(const adsb_modes_rec &r)
{
    const uint32_t df = r.df;
    uint32_t w = 0;
    if (r.flags & ADSB_MODES_ALT) w |= kModesAlt;
    if (r.flags & ADSB_MODES_SQUAWK) w |= kModesSquawk;
    if (r.flags & ADSB_MODES_CALLSIGN) w |= kModesCallsign;
    if (modes_squitter(df)) return w | kModesSquitter;
    w |= kModesReply;
    if (df == 11) w |= kModesAllcall;
    if (df == 4 || df == 5 || df == 20 || df == 21) w |= kModesSurveillance | kModesStatus | kModesGround;
    if (df == 0 || df == 16) w |= kModesAirAir | kModesGround;
    return w;
}

// The 64 bytes of a modes record as words, for stores and moves
struct ModesWords {
    uint64_t w[8];
};

// The empty record: the three times NaN, all else zero
ADSB_HD inline adsb_aircraft_modes modes_empty_record()
{
    adsb_aircraft_modes a;
    __builtin_memset(&a, 0, sizeof(a));
    a.altitude_time = a.squawk_time = a.callsign_time = __builtin_nan("");
    return a;
}

ADSB_HD inline ModesWords modes_empty()
{
    const adsb_aircraft_modes a = modes_empty_record();
    ModesWords o;
    __builtin_memcpy(&o, &a, sizeof(o));
    return o;
}

// The counts and the squitter bit of a run of counted frames
struct ModesCounts {
    uint32_t n_replies, n_allcall, n_surveillance, n_airair, squitter;
};

// The record of a run of counted frames that starts from nothing: its counts, and the run's newest frame of each sort
// (null: the run has none) with the time of the three that carry one.  `any` is the run's newest frame of any DF.
ADSB_HD inline adsb_aircraft_modes modes_part(const ModesCounts &c, const adsb_modes_rec *any, const adsb_modes_rec *alt,
                                              double t_alt, const adsb_modes_rec *squawk, double t_squawk,
                                              const adsb_modes_rec *callsign, double t_callsign,
                                              const adsb_modes_rec *status, const adsb_modes_rec *ground)
{
    adsb_aircraft_modes a = modes_empty_record();
    uint32_t flags = c.squitter ? ADSB_TRACK_MODES_SQUITTER : 0u;
    a.n_replies = c.n_replies;
    a.n_allcall = c.n_allcall;
    a.n_surveillance = c.n_surveillance;
    a.n_airair = c.n_airair;
    if (any) a.last_df = any->df;
    if (alt) {
        a.altitude_ft = alt->altitude_ft;
        a.altitude_time = t_alt;
        flags |= ADSB_TRACK_MODES_ALT;
    }
    if (squawk) {
        a.squawk = squawk->squawk;
        a.squawk_time = t_squawk;
        flags |= ADSB_TRACK_MODES_SQUAWK;
    }
    if (callsign) {
        __builtin_memcpy(a.callsign, callsign->callsign, 8);
        a.callsign_time = t_callsign;
        flags |= ADSB_TRACK_MODES_CALLSIGN;
    }
    if (status) {
        a.fs = status->fs;
        flags |= ADSB_TRACK_MODES_STATUS | (status->flags & (ADSB_MODES_ALERT | ADSB_MODES_SPI));
    }
    if (ground) flags |= ground->flags & ADSB_MODES_GROUND;
    a.flags = (uint16_t)flags;
    return a;
}

ADSB_HD inline uint32_t modes_sat_add(uint32_t a, uint32_t b)
{
    const uint32_t c = a + b;
    return c < a ? ~0u : c;
}

// `into` followed by `later`, a record made by modes_part (or by this function) over the frames that come after
// into's.  A part says which fields it holds by its flags; it has a source of GROUND iff it counted a DF0/4/5/16/20/21
// frame, and a newest frame iff it counted any.  Associative; the empty record is its identity.
ADSB_HD inline void modes_merge(adsb_aircraft_modes &into, const adsb_aircraft_modes &later)
{
    uint32_t flags = into.flags;
    if (later.flags & ADSB_TRACK_MODES_ALT) {
        into.altitude_ft = later.altitude_ft;
        into.altitude_time = later.altitude_time;
        flags |= ADSB_TRACK_MODES_ALT;
    }
    if (later.flags & ADSB_TRACK_MODES_SQUAWK) {
        into.squawk = later.squawk;
        into.squawk_time = later.squawk_time;
        flags |= ADSB_TRACK_MODES_SQUAWK;
    }
    if (later.flags & ADSB_TRACK_MODES_CALLSIGN) {
        __builtin_memcpy(into.callsign, later.callsign, 8);
        into.callsign_time = later.callsign_time;
        flags |= ADSB_TRACK_MODES_CALLSIGN;
    }
    if (later.flags & ADSB_TRACK_MODES_STATUS) {
        into.fs = later.fs;
        flags = (flags & ~(ADSB_TRACK_MODES_ALERT | ADSB_TRACK_MODES_SPI)) | ADSB_TRACK_MODES_STATUS |
                (later.flags & (ADSB_TRACK_MODES_ALERT | ADSB_TRACK_MODES_SPI));
    }
    if (later.n_surveillance || later.n_airair) // saturated counts stay non-zero
        flags = (flags & ~ADSB_TRACK_MODES_GROUND) | (later.flags & ADSB_TRACK_MODES_GROUND);
    flags |= later.flags & ADSB_TRACK_MODES_SQUITTER;
    if (later.n_replies || (later.flags & ADSB_TRACK_MODES_SQUITTER)) into.last_df = later.last_df;
    into.n_replies = modes_sat_add(into.n_replies, later.n_replies);
    into.n_allcall = modes_sat_add(into.n_allcall, later.n_allcall);
    into.n_surveillance = modes_sat_add(into.n_surveillance, later.n_surveillance);
    into.n_airair = modes_sat_add(into.n_airair, later.n_airair);
    into.flags = (uint16_t)flags;
    for (int k = 0; k < 6; ++k) into.reserved[k] = 0;
}

// The record of an aircraft whose only counted frame is this ACCEPTED one
ADSB_HD inline adsb_aircraft_modes modes_one(const adsb_modes_rec &r, double time)
{
    const uint32_t w = modes_what(r);
    ModesCounts c;
    c.n_replies = (w & kModesReply) ? 1u : 0u;
    c.n_allcall = (w & kModesAllcall) ? 1u : 0u;
    c.n_surveillance = (w & kModesSurveillance) ? 1u : 0u;
    c.n_airair = (w & kModesAirAir) ? 1u : 0u;
    c.squitter = (w & kModesSquitter) ? 1u : 0u;
    return modes_part(c, &r, (w & kModesAlt) ? &r : nullptr, time, (w & kModesSquawk) ? &r : nullptr, time,
                      (w & kModesCallsign) ? &r : nullptr, time, (w & kModesStatus) ? &r : nullptr,
                      (w & kModesGround) ? &r : nullptr);
}

} // namespace adsbk
#endif
