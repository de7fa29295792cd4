// adsb_wire.cpp -- CPU mirror of the device's wire output (adsb_wire.hip): adsb_host_wire_encode of include/adsb_host.h.
// The encoder itself is ../adsb_wire.h, the text the device compiles; here only the loop over the list.  No device.
#include "../../../include/adsb_host.h"
#include "../adsb_wire.h"

#include <cstring>

extern "C" int adsb_host_wire_encode(const adsb_wire_cfg *cfg, int sample_type, const adsb_frame *frames,
                                     const adsb_frame_level *levels, size_t n, uint8_t *out, size_t cap, size_t *n_bytes,
                                     uint32_t *ends)
{
    if (!adsbk::wire_cfg_ok(cfg) || !n_bytes || (!frames && n) || (!out && cap)) return ADSB_E_ARG;
    if (sample_type != ADSB_SAMPLE_I8 && sample_type != ADSB_SAMPLE_I16) return ADSB_E_ARG;
    if ((uint64_t)n * adsbk::kWireMaxBytes > 0xFFFFFFFFull) return ADSB_E_CAPACITY;
    const bool with_signal = cfg->signal != 0 && adsbk::wire_base_format(cfg->format) == ADSB_WIRE_BEAST && levels;
    size_t total = 0;
    bool fits = true; // whole frames only: the first frame that does not fit ends the copy, not the count
    for (size_t i = 0; i < n; ++i) {
        const uint64_t t = adsbk::wire_ticks(frames[i].offset, cfg->tick_bias);
        const uint32_t s = with_signal ? adsbk::wire_signal_of(&levels[i], sample_type, cfg->format) : 0u;
        uint8_t one[adsbk::kWireMaxBytes];
        const uint32_t len = adsbk::wire_encode(cfg->format, t, s, frames[i].bytes, one);
        fits = fits && total + len <= cap;
        if (fits) std::memcpy(out + total, one, len);
        total += len;
        if (ends) ends[i] = (uint32_t)total;
    }
    *n_bytes = total;
    return ADSB_OK;
}
