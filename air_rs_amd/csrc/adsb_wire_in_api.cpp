// adsb_wire_in_api.cpp -- the C boundary of the wire input (include/adsb_hip.h, "Wire input"): argument checks, the one
// device block the kernels' arrays are carved from, the copy of a host input, and the fetch.  The kernels are
// adsb_wire_in.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "adsb_scratch.h"
#include "adsb_wire_in.h"

// One block for an input of `bytes` bytes and `frames` kept frames.  Every array starts 256-byte aligned.
static int win_reserve(adsb_ctx *c, size_t bytes, size_t frames, bool levels)
{
    adsb_ctx::WireIn &k = c->win;
    if (k.mem.p && k.bytes >= bytes && k.frames >= frames && (k.levels || !levels)) return ADSB_OK;
    bytes = std::max(bytes, k.bytes);
    frames = std::max(frames, k.frames);
    levels = levels || k.levels;
    k.bytes = k.frames = 0;
    k.levels = k.done = false;
    const size_t f = std::max<size_t>(frames, 1);
    const size_t spans = (size_t)adsbk::wire_in_spans((uint64_t)bytes + 3) + 1; // whatever the input's alignment
    const int rc = carve_block(c, k.mem, [&k, f, spans, levels](Carve &cv) {
        adsbk::WireInArgs &a = k.a;
        a = adsbk::WireInArgs{};
        a.last = cv.take<uint32_t>(spans);
        a.carry = cv.take<uint64_t>(spans);
        a.tally = cv.take<adsbk::WireInTally>(spans);
        a.inc = cv.take<uint32_t>(adsbk::kWireInMaxStreams);
        a.tail = cv.take<uint32_t>(adsbk::kWireInMaxStreams);
        k.ends = cv.take<uint32_t>(adsbk::kWireInMaxStreams);
        a.frames = cv.take<adsb_frame>(f);
        a.rx = cv.take<adsb_wire_rx>(f);
        a.levels = levels ? cv.take<adsb_frame_level>(f) : nullptr;
        a.counts = cv.take<uint64_t>(adsbk::kWireInMaxStreams);
        a.consumed = cv.take<uint64_t>(adsbk::kWireInMaxStreams);
        a.hdr = cv.take<adsb_wire_in_header>(1);
    });
    if (rc != ADSB_OK) return rc;
    k.bytes = bytes;
    k.frames = frames;
    k.levels = levels;
    return ADSB_OK;
}

// The checked ends of the streams as 32-bit words; ADSB_E_ARG / ADSB_E_CAPACITY as adsb_wire_in_of documents.  Shared
// with nothing: the CPU mirror checks the same in its own file, without the HIP runtime.
static int win_check(const adsb_wire_in_cfg *cfg, const uint8_t *bytes, size_t n_bytes, const uint64_t *stream_ends,
                     uint32_t n_streams, std::vector<uint32_t> *ends)
{
    if (!adsbk::wire_in_cfg_ok(cfg) || !stream_ends || (!bytes && n_bytes) || n_streams < 1 ||
        n_streams > adsbk::kWireInMaxStreams)
        return ADSB_E_ARG;
    if ((uint64_t)n_bytes > 0xFFFFFFFFull) return ADSB_E_CAPACITY;
    ends->resize(n_streams);
    uint64_t prev = 0;
    for (uint32_t r = 0; r < n_streams; ++r) {
        if (stream_ends[r] < prev || stream_ends[r] > (uint64_t)n_bytes) return ADSB_E_ARG;
        (*ends)[r] = (uint32_t)(prev = stream_ends[r]);
    }
    return prev == (uint64_t)n_bytes ? ADSB_OK : ADSB_E_ARG;
}

extern "C" int adsb_wire_in_of(adsb_ctx *c, const adsb_wire_in_cfg *cfg, const uint8_t *bytes, size_t n_bytes,
                               const uint64_t *stream_ends, uint32_t n_streams)
{
    if (!c) return ADSB_E_ARG;
    std::vector<uint32_t> ends;
    int rc = win_check(cfg, bytes, n_bytes, stream_ends, n_streams, &ends);
    if (rc != ADSB_OK) return rc;
    HIPCHK(hipSetDevice(c->cfg.device));
    const size_t most = (size_t)adsbk::wire_in_most(cfg->filter, n_bytes); // frames that can exist
    const size_t cap = cfg->max_frames ? (size_t)std::min<uint64_t>(cfg->max_frames, most) : most;
    if ((rc = win_reserve(c, n_bytes, cap, cfg->levels != 0)) != ADSB_OK) return rc;
    adsb_ctx::WireIn &k = c->win;
    const uint8_t *in = bytes;
    if (n_bytes && !in_device_memory(c, bytes)) {
        if ((rc = grow(c, k.in, (n_bytes + 3) & ~(size_t)3)) != ADSB_OK) return rc; // whole dwords
        HIPCHK(hipMemcpyAsync(k.in.p, bytes, n_bytes, hipMemcpyHostToDevice, c->aux));
        in = k.in.p;
    }
    HIPCHK(hipMemcpyAsync(k.ends, ends.data(), sizeof(uint32_t) * n_streams, hipMemcpyHostToDevice, c->aux));
    HIPCHK(hipStreamSynchronize(c->aux)); // the host arrays are the caller's (and this frame's) again
    adsbk::WireInArgs a = k.a;
    a.lead = n_bytes ? (uint32_t)((uintptr_t)in & 3u) : 0u;
    a.words = n_bytes ? (const uint32_t *)((uintptr_t)in - a.lead) : (const uint32_t *)k.ends; // (not read when empty)
    a.n_bytes = (uint32_t)n_bytes;
    a.n_streams = n_streams;
    a.ends = k.ends;
    a.format = cfg->format;
    a.filter = cfg->filter;
    a.tick_bias = cfg->tick_bias;
    a.sample_type = cfg->sample_type;
    a.cap = (uint32_t)cap;
    a.n_spans = adsbk::wire_in_spans((uint64_t)a.lead + n_bytes);
    if (!cfg->levels) a.levels = nullptr;
    HIPCHK(adsbk::launch_wire_in(c->aux, a));
    k.n_streams = n_streams;
    k.with_levels = cfg->levels != 0;
    k.done = true;
    return ADSB_OK;
}

extern "C" int adsb_fetch_wire_in(adsb_ctx *c, adsb_frame *frames, adsb_wire_rx *rx, adsb_frame_level *levels, size_t max,
                                  size_t *n, uint64_t *counts, uint64_t *consumed, uint32_t n_streams,
                                  adsb_wire_in_header *header)
{
    if (!c) return ADSB_E_ARG;
    const adsb_ctx::WireIn &k = c->win;
    if (!k.done || (levels && !k.with_levels)) return ADSB_E_STATE;
    if (n_streams > k.n_streams) return ADSB_E_ARG;
    HIPCHK(hipSetDevice(c->cfg.device));
    adsb_wire_in_header h{};
    HIPCHK(hipMemcpyAsync(&h, k.a.hdr, sizeof(h), hipMemcpyDeviceToHost, c->aux));
    HIPCHK(hipStreamSynchronize(c->aux));
    const size_t m = std::min<size_t>((size_t)h.n_frames, max);
    if (m && frames) HIPCHK(hipMemcpyAsync(frames, k.a.frames, sizeof(adsb_frame) * m, hipMemcpyDeviceToHost, c->aux));
    if (m && rx) HIPCHK(hipMemcpyAsync(rx, k.a.rx, sizeof(adsb_wire_rx) * m, hipMemcpyDeviceToHost, c->aux));
    if (m && levels) HIPCHK(hipMemcpyAsync(levels, k.a.levels, sizeof(adsb_frame_level) * m, hipMemcpyDeviceToHost, c->aux));
    if (n_streams && counts) HIPCHK(hipMemcpyAsync(counts, k.a.counts, 8 * (size_t)n_streams, hipMemcpyDeviceToHost, c->aux));
    if (n_streams && consumed)
        HIPCHK(hipMemcpyAsync(consumed, k.a.consumed, 8 * (size_t)n_streams, hipMemcpyDeviceToHost, c->aux));
    HIPCHK(hipStreamSynchronize(c->aux));
    if (n) *n = m;
    if (header) *header = h;
    return ADSB_OK;
}

extern "C" int adsb_wire_in_device(adsb_ctx *c, const adsb_frame **frames_dev, const adsb_wire_rx **rx_dev,
                                   const adsb_frame_level **levels_dev, const uint64_t **counts_dev,
                                   const uint64_t **consumed_dev, const void **header_dev)
{
    if (!c) return ADSB_E_ARG;
    const adsb_ctx::WireIn &k = c->win;
    if (!k.done) return ADSB_E_STATE;
    if (frames_dev) *frames_dev = k.a.frames;
    if (rx_dev) *rx_dev = k.a.rx;
    if (levels_dev) *levels_dev = k.with_levels ? k.a.levels : nullptr;
    if (counts_dev) *counts_dev = k.a.counts;
    if (consumed_dev) *consumed_dev = k.a.consumed;
    if (header_dev) *header_dev = k.a.hdr;
    return ADSB_OK;
}

extern "C" int adsb_debug_wire_in_geometry(uint32_t *bytes_per_block, uint32_t *scan_threads)
{
    if (bytes_per_block) *bytes_per_block = adsbk::kWireInBlockBytes;
    if (scan_threads) *scan_threads = adsbk::kWireInScanThreads;
    return ADSB_OK;
}
