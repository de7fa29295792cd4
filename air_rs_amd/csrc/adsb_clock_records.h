// adsb_clock_records.h -- the sizes and records of clock sync that the kernels' arguments and the context hold
// (adsb_kernels.h); adsb_clock.h has the text that works on them.  Internal.
#ifndef ADSB_CLOCK_RECORDS_H
#define ADSB_CLOCK_RECORDS_H

#include "adsb_mlat.h"

namespace adsbk {

constexpr uint32_t kClockLanes = kMlatLanes;   // lanes per message of the rows and apply kernels
constexpr uint32_t kClockPartials = 64;        // partial sums of a pair: one wavefront
constexpr uint32_t kClockEmpty = 0xFFFFFFFFu;  // an empty slot's key; bit 16 set, so it sorts last on 17 bits
constexpr uint32_t kClockKeyBits = 17;
constexpr uint32_t kClockMaxUnknowns = 2 * (kMlatMaxReceivers - 1);

// A receiver as the rows see it: the solver's station (clock = the prior) and where the position decode stands.
struct ClockStation {
    MlatStation s;
    double latitude, longitude;
};

// A pair's sums over its rows.
struct ClockPair {
    double st, stt, sy, sty, syy;
    uint64_t n;
};

// A receiver's solution: what the residuals and apply read.
struct ClockSol {
    double a, b;
};

static_assert(sizeof(adsb_clock_cfg) == 64 && sizeof(adsb_clock) == 64 && sizeof(adsb_clock_header) == 64 &&
                  sizeof(ClockStation) == 48 && sizeof(ClockPair) == 48,
              "clock records");

// The cfg with its defaults filled in.
struct ClockParams {
    uint32_t time_source, flags, reference, min_rows;
    double seconds_per_tick, seconds_per_time, max_residual_s, max_range_nm;
};

} // namespace adsbk

#endif
