// adsb_fix.cpp -- CPU mirror of the tracker's per-frame fix decode: adsb_host_fix_of of include/adsb_host.h.  The decode
// itself is ../adsb_fix.h, the text the device compiles; here only the one-frame merge around it.  No device.
#include "../../../include/adsb_host.h"
#include "../adsb_fix.h"

#include <cstring>

extern "C" int adsb_host_fix_of(const adsb_site *site, const uint8_t bytes[14], double time, adsb_fix *out,
                                uint32_t *frame_flags)
{
    if (!site || !bytes || !out || !adsbk::fix_site_ok(*site)) return ADSB_E_ARG;
    adsb_frame_fix f;
    adsbk::FixRem r;
    adsbk::fix_decode(*site, bytes, f, r);
    const adsbk::FixWords empty = adsbk::fix_empty();
    adsb_fix a;
    std::memcpy(&a, &empty, sizeof(a));
    if (f.flags & ADSB_FIX_VALID) {
        adsbk::fix_take(a, f, r, time);
        a.n_fixes = 1;
    } else if (f.flags & ADSB_FIX_REJECTED) {
        a.n_rejected = 1;
    }
    std::memcpy(out, &a, sizeof(a));
    if (frame_flags) *frame_flags = f.flags;
    return ADSB_OK;
}
