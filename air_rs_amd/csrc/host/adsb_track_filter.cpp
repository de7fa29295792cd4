// adsb_track_filter.cpp -- CPU mirror of the track table's filter behind its multilaterated fixes:
// adsb_host_track_filter_operand and adsb_host_track_filter_step of include/adsb_host.h.  The text is
// ../adsb_track_filter.h, which the device compiles too; here only the argument checks around it.  No device.
#include "../../../include/adsb_host.h"
#include "../adsb_track_filter.h"

extern "C" int adsb_host_track_filter_operand(const adsb_track_filter_cfg *cfg, const adsb_mlat_fix *fix, double time,
                                              int counted, adsb_filter_operand *operand)
{
    adsb_track_filter_cfg use;
    if (!fix || !operand || !adsbk::filter_cfg_resolve(cfg, use)) return ADSB_E_ARG;
    *operand = adsbk::filter_operand(use, *fix, time, counted != 0);
    return ADSB_OK;
}

extern "C" int adsb_host_track_filter_step(const adsb_track_filter_cfg *cfg, adsb_aircraft_filter *record,
                                           const adsb_filter_operand *operand, adsb_frame_filter *frame_out)
{
    adsb_track_filter_cfg use;
    if (!record || !operand || !adsbk::filter_cfg_resolve(cfg, use)) return ADSB_E_ARG;
    adsb_frame_filter f;
    adsbk::filter_step(use, *record, *operand, f);
    if (frame_out) *frame_out = f;
    return ADSB_OK;
}
