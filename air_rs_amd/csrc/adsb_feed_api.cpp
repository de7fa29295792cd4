// adsb_feed_api.cpp -- the streaming front end of the C boundary (adsb_feed_* of include/adsb_hip.h) and the two
// measurements that are clients of it and of the public API only.  What it needs from adsb_api.cpp is declared in
// adsb_ctx.h: the one-dispatch path for small buffers and the view of the older of two launches in flight.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <new>
#include <vector>

#include "adsb_ctx.h"

using adsbk::kWindow;

// ---- streaming front end (reference: the Vec-per-recv loop of src/adsb.rs:95-98 and its feeders,
// adsb.rs:54-89) --------------------------------------------------------------------------------------------
// Buffers arrive on the host one after the other.  Each is copied into a slot of a PINNED host ring (or was
// written there by the producer: adsb_feed_acquire), goes to one of two device staging slots by asynchronous DMA
// on a copy stream, and is demodulated on the ctx stream -- so the copy of buffer k+1 overlaps the kernels of
// buffer k, and the host only blocks in adsb_feed_pop() for results that are not ready yet.  Two buffers may be
// in flight (the ctx alternates between two result sets).
//   parity mode (carry = 0, the reference's behaviour): every buffer is its own reference buffer; the last 240
//     offsets of each are never looked at (adsb.rs:98); offsets are buffer-relative.
//   carry mode (carry = 1): the last 240 samples of the stream so far are kept ON THE DEVICE and copied, device
//     to device, in front of the next buffer before it is demodulated: the chunked stream decodes exactly like one
//     long buffer (frames straddling two buffers are found); offsets are absolute stream positions.
// Staging slot layout (samples): [ head: up to 240 carried samples | the buffer ], the buffer's copy lands behind
// the carried samples and the demodulated region starts at a multiple of 8 samples (16-byte alignment).
struct adsb_feed {
    adsb_ctx *c = nullptr;
    adsb_feed_cfg cfg{};
    uint32_t bps = 2;
    hipStream_t copy = nullptr;
    char *dev[2] = {nullptr, nullptr};
    hipEvent_t h2d_done[2] = {nullptr, nullptr}, kern_done[2] = {nullptr, nullptr};
    // results of the launch from staging slot k are complete and visible to the copy engine (a default event: its
    // record releases to system scope, unlike the ctx's device-scope events)
    bool kern_pending[2] = {false, false};
    std::vector<char *> ring;
    std::vector<hipEvent_t> ring_done; // H2D out of that ring slot has completed
    std::vector<char> ring_busy;
    // a one-dispatch launch reads its samples straight from the ring slot: the slot may be overwritten once the launch's
    // sequence word says so (ring_seq != 0: result set ring_set carries that number when the kernel has finished) AND, if
    // its buffer is still unpopped, its list is complete -- a re-run after a slot-pool overflow reads the slot again
    std::vector<uint64_t> ring_seq;
    std::vector<uint32_t> ring_set;
    uint32_t ring_next = 0;
    int acquired = -1;
    uint64_t pushed = 0, popped = 0; // buffers
    uint64_t consumed = 0;           // samples pushed so far
    size_t prev_start = 0, prev_len = 0; // demodulated region of the previous buffer's slot (samples)
    struct Entry {
        bool launched = false;
        bool small = false;        // went through the one-dispatch path: results in the ctx's pinned blob `set`
        uint64_t seq = 0;          // ... complete when its sequence word carries this
        uint32_t set = 0;
        uint64_t first_sample = 0; // stream position of the buffer's first own sample
    } q[2];
    adsbk::Header *hdr_host = nullptr;
    size_t headroom = 0;           // samples in front of every ring slot's data (carry mode: room for the 240-sample tail)
    const char *prev_host = nullptr; // where the previous buffer's demodulated region starts in HOST memory (nullptr: it
                                     // only exists in a device staging slot)
    uint32_t prev_ring = 0;          // ... and the ring slot that holds it
};

extern "C" void adsb_feed_close(adsb_feed *f)
{
    if (!f) return;
    if (f->c) (void)hipSetDevice(f->c->cfg.device);
    if (f->copy) (void)hipStreamSynchronize(f->copy);
    if (f->c && f->c->stream) (void)hipStreamSynchronize(f->c->stream);
    for (int k = 0; k < 2; ++k) {
        (void)hipFree(f->dev[k]);
        if (f->h2d_done[k]) (void)hipEventDestroy(f->h2d_done[k]);
        if (f->kern_done[k]) (void)hipEventDestroy(f->kern_done[k]);
    }
    for (char *p : f->ring) (void)hipHostFree(p);
    for (hipEvent_t e : f->ring_done) if (e) (void)hipEventDestroy(e);
    if (f->hdr_host) (void)hipHostFree(f->hdr_host);
    if (f->copy) (void)hipStreamDestroy(f->copy);
    if (f->c) { (void)adsb_set_stream_base(f->c, 0); }
    delete f;
}

extern "C" int adsb_feed_open(adsb_ctx *c, const adsb_feed_cfg *cfg, adsb_feed **out)
{
    if (!c || !cfg || !out || cfg->max_chunk == 0) return ADSB_E_ARG;
    *out = nullptr;
    // one launch covers the buffer, in carry mode with the 240 carried samples in front of it
    if (cfg->max_chunk + (cfg->carry ? (size_t)kWindow : 0) > c->cfg.max_samples) return ADSB_E_CAPACITY;
    if (c->cfg.max_channels < 1) return ADSB_E_ARG;
    // two launches are in flight: they must not share one caller-owned result blob
    if (c->ext_blob) return ADSB_E_STATE;
    HIPCHK(hipSetDevice(c->cfg.device));
    adsb_feed *f = new (std::nothrow) adsb_feed();
    if (!f) return ADSB_E_NOMEM;
    f->c = c;
    f->cfg = *cfg;
    if (f->cfg.ring_slots < 2) f->cfg.ring_slots = 3;
    f->bps = c->bps;
    bool ok = hipStreamCreateWithFlags(&f->copy, hipStreamNonBlocking) == hipSuccess;
    f->headroom = kWindow; // (240 samples = 480 / 960 bytes: keeps the data 16-byte aligned)
    const size_t slot_bytes = (cfg->max_chunk + (size_t)kWindow + 8) * f->bps;
    for (int k = 0; k < 2 && ok; ++k)
        ok = hipMalloc((void **)&f->dev[k], slot_bytes) == hipSuccess &&
             hipEventCreateWithFlags(&f->h2d_done[k], hipEventDisableTiming) == hipSuccess &&
             hipEventCreateWithFlags(&f->kern_done[k], hipEventDisableTiming) == hipSuccess;
    for (uint32_t k = 0; k < f->cfg.ring_slots && ok; ++k) {
        char *p = nullptr;
        hipEvent_t e = nullptr;
        ok = hipHostMalloc((void **)&p, (cfg->max_chunk + f->headroom) * f->bps, hipHostMallocDefault) == hipSuccess &&
             hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess;
        if (p) f->ring.push_back(p);
        if (e) f->ring_done.push_back(e);
        f->ring_busy.push_back(0);
        f->ring_seq.push_back(0);
        f->ring_set.push_back(0);
    }
    ok = ok && hipHostMalloc((void **)&f->hdr_host, sizeof(adsbk::Header), hipHostMallocDefault) == hipSuccess;
    if (!ok) { adsb_feed_close(f); return ADSB_E_NOMEM; }
    *out = f;
    return ADSB_OK;
}

extern "C" int adsb_feed_in_flight(const adsb_feed *f) { return f ? (int)(f->pushed - f->popped) : ADSB_E_ARG; }

// 1: adsb_feed_pop() would not wait for the GPU (the oldest buffer's kernels have finished, or it launched none);
// 0: it would; ADSB_E_STATE: nothing in flight.
extern "C" int adsb_feed_ready(adsb_feed *f)
{
    if (!f) return ADSB_E_ARG;
    if (f->popped == f->pushed) return ADSB_E_STATE;
    const uint32_t s = (uint32_t)(f->popped & 1u);
    if (!f->q[s].launched) return 1;
    if (f->q[s].small) return small_reached(f->c, f->q[s].set, f->q[s].seq) ? 1 : 0;
    HIPCHK(hipSetDevice(f->c->cfg.device));
    const hipError_t e = hipEventQuery(f->kern_done[s]);
    if (e == hipSuccess) return 1;
    if (e == hipErrorNotReady) { (void)hipGetLastError(); return 0; }
    return (int)e;
}

static int feed_ring_slot(adsb_feed *f, uint32_t *slot)
{
    const uint32_t r = f->ring_next;
    if (f->ring_busy[r]) { // the DMA out of this slot must have finished before the host overwrites it
        HIPCHK(hipEventSynchronize(f->ring_done[r]));
        f->ring_busy[r] = 0;
    }
    if (f->ring_seq[r]) { // ... and so must the one-dispatch kernel that reads its samples from the slot itself
        const int rc = small_wait(f->c, f->ring_set[r], f->ring_seq[r], true);
        if (rc != ADSB_OK) return rc;
        // ... and, while that buffer has not been popped, so must its LIST: a launch whose tiles lost their slots is
        // re-run from these samples (small_complete), which the pop would otherwise do after the producer has overwritten
        // them.  (Unpopped means no later launch has used its result set: the sequence word is exactly this launch's.)
        for (uint64_t k = f->popped; k < f->pushed; ++k) {
            const adsb_feed::Entry &e = f->q[k & 1u];
            if (!e.launched || !e.small || e.set != f->ring_set[r] || e.seq != f->ring_seq[r]) continue;
            const int rc2 = small_complete(f->c, e.set);
            if (rc2 != ADSB_OK) return rc2;
        }
        f->ring_seq[r] = 0;
    }
    *slot = r;
    return ADSB_OK;
}

extern "C" int adsb_feed_acquire(adsb_feed *f, void **host_slot)
{
    if (!f || !host_slot) return ADSB_E_ARG;
    if (f->acquired >= 0) return ADSB_E_STATE;
    HIPCHK(hipSetDevice(f->c->cfg.device));
    uint32_t r = 0;
    int rc = feed_ring_slot(f, &r);
    if (rc != ADSB_OK) return rc;
    f->acquired = (int)r;
    *host_slot = f->ring[r] + f->headroom * f->bps;
    return ADSB_OK;
}

extern "C" int adsb_feed_push(adsb_feed *f, const void *iq_host, size_t n)
{
    if (!f || n == 0 || n > f->cfg.max_chunk) return ADSB_E_ARG;
    if (!iq_host && f->acquired < 0) return ADSB_E_ARG;
    if (f->pushed - f->popped >= 2) return ADSB_E_STATE; // two buffers in flight: pop first
    // parity mode: the reference panics on a buffer shorter than 240 samples (adsb.rs:98); nothing is consumed
    if (!f->cfg.carry && n < (size_t)kWindow) return ADSB_E_SHORT;
    adsb_ctx *c = f->c;
    HIPCHK(hipSetDevice(c->cfg.device));
    uint32_t r = 0;
    char *data = nullptr; // the buffer's samples in the pinned ring
    if (f->acquired >= 0) {
        r = (uint32_t)f->acquired;
        data = f->ring[r] + f->headroom * f->bps;
        if (iq_host && iq_host != data) std::memcpy(data, iq_host, n * f->bps);
        f->acquired = -1;
    } else {
        int rc = feed_ring_slot(f, &r);
        if (rc != ADSB_OK) return rc;
        data = f->ring[r] + f->headroom * f->bps;
        std::memcpy(data, iq_host, n * f->bps);
    }
    f->ring_next = (r + 1) % (uint32_t)f->ring.size();

    const uint32_t s = (uint32_t)(f->pushed & 1u);
    const size_t tail = (f->cfg.carry && f->pushed) ? std::min<size_t>(kWindow, f->prev_len) : 0;
    const size_t len = tail + n;
    adsb_feed::Entry &e = f->q[s];
    e.first_sample = f->consumed;
    e.launched = false;
    e.small = false;
    const uint64_t base = f->cfg.carry ? f->consumed - tail : 0;

    // ---- small buffers: one dispatch, samples read from the ring and frames written to pinned memory by the device ----
    // (carry mode: the tail of the previous buffer is copied in front of this one on the host -- 480 or 960 bytes --
    // which needs that buffer in host memory and a 16-byte aligned start, i.e. the usual 240-sample tail)
    if (len >= (size_t)kWindow && small_fits(c, len) && (tail == 0 || (f->prev_host && (tail * f->bps) % 16 == 0))) {
        char *start = data - tail * f->bps;
        if (tail) std::memcpy(start, f->prev_host + (f->prev_len - tail) * f->bps, tail * f->bps);
        int rc = adsb_set_stream_base(c, base);
        if (rc == ADSB_OK) rc = small_launch(c, start, len, &e.seq);
        if (rc != ADSB_OK) return rc;
        e.launched = true;
        e.small = true;
        e.set = c->last;
        f->ring_busy[r] = 0;
        f->ring_seq[r] = e.seq; // the kernel reads the slot until its sequence word is out (feed_ring_slot waits for it)
        f->ring_set[r] = e.set;
        f->prev_host = start;
        f->prev_ring = r;
        f->prev_start = 0;
        f->prev_len = len;
        f->consumed += n;
        f->pushed++;
        return ADSB_OK;
    }

    const size_t start = ((size_t)kWindow - tail) / 8 * 8; // 16-byte aligned start of the demodulated region
    // this staging slot was last read by the launch two buffers ago
    if (f->kern_pending[s]) HIPCHK(hipStreamWaitEvent(f->copy, f->kern_done[s], 0));
    HIPCHK(hipMemcpyAsync(f->dev[s] + (start + tail) * f->bps, data, n * f->bps, hipMemcpyHostToDevice, f->copy));
    HIPCHK(hipEventRecord(f->ring_done[r], f->copy));
    f->ring_busy[r] = 1;
    if (tail) { // the last `tail` samples of what the previous launch saw
        if (f->prev_host) { // ... which went through the one-dispatch path: they are in the ring (host memory)
            HIPCHK(hipMemcpyAsync(f->dev[s] + start * f->bps, f->prev_host + (f->prev_len - tail) * f->bps, tail * f->bps,
                                  hipMemcpyHostToDevice, f->copy));
            HIPCHK(hipEventRecord(f->ring_done[f->prev_ring], f->copy)); // that slot is read once more: not reusable before
            f->ring_busy[f->prev_ring] = 1;
        } else // ... device to device (its H2D is earlier on this stream)
            HIPCHK(hipMemcpyAsync(f->dev[s] + start * f->bps, f->dev[s ^ 1u] + (f->prev_start + f->prev_len - tail) * f->bps,
                                  tail * f->bps, hipMemcpyDeviceToDevice, f->copy));
    }
    HIPCHK(hipEventRecord(f->h2d_done[s], f->copy));

    if (len >= (size_t)kWindow) {
        HIPCHK(hipStreamWaitEvent(c->stream, f->h2d_done[s], 0));
        // after a pop of an older launch the ctx may "view" that launch: the next enqueue starts from the newest state
        int rc = adsb_set_stream_base(c, base);
        if (rc == ADSB_OK) rc = adsb_demod_device_async(c, f->dev[s] + start * f->bps, 1, len, len);
        if (rc != ADSB_OK) return rc;
        e.launched = true;
        e.set = c->last;
        HIPCHK(hipEventRecord(f->kern_done[s], c->aux)); // THIS launch's kernels and results (not the stream's tail)
        f->kern_pending[s] = true;
    }
    f->prev_host = nullptr;
    f->prev_start = start;
    f->prev_len = len;
    f->consumed += n;
    f->pushed++;
    return ADSB_OK;
}

extern "C" int adsb_feed_pop(adsb_feed *f, adsb_frame *out, size_t max_out, size_t *n_out, uint32_t *flags,
                             uint64_t *first_sample)
{
    if (!f || !n_out || (!out && max_out)) return ADSB_E_ARG;
    *n_out = 0;
    if (flags) *flags = 0;
    if (f->popped == f->pushed) return ADSB_E_STATE;
    adsb_ctx *c = f->c;
    HIPCHK(hipSetDevice(c->cfg.device));
    adsb_feed::Entry &e = f->q[f->popped & 1u];
    if (first_sample) *first_sample = e.first_sample;
    f->popped++;
    if (!e.launched) return ADSB_OK; // (carry mode, fewer than 240 samples so far: nothing decodable yet)
    if (e.small) { // the device wrote header and frames into pinned memory: poll its sequence word, copy, done
        int rc = small_wait(c, e.set, e.seq);
        if (rc != ADSB_OK) return rc;
        return small_collect(c, e.set, out, max_out, n_out, nullptr, flags);
    }
    adsb_ctx::ResultSet &r = c->rs[e.set];
    // results travel on the copy stream, behind this launch's ordering pass only -- not behind the kernels of the
    // buffer pushed after it, which share the ctx stream
    HIPCHK(hipStreamWaitEvent(f->copy, f->kern_done[(f->popped - 1) & 1u], 0));
    HIPCHK(hipMemcpyAsync(f->hdr_host, r.hdr, sizeof(adsbk::Header), hipMemcpyDeviceToHost, f->copy));
    HIPCHK(hipStreamSynchronize(f->copy));
    if (f->hdr_host->retry) { // slot-pool overflow (pathological input): the slow, fully synchronous path
        // (adsb_fetch writes *n_out and *flags only when it succeeds: they stay 0 otherwise)
        return with_launch_in_view(c, e.set, [&] { return adsb_fetch(c, out, max_out, n_out, nullptr, nullptr, flags); });
    }
    uint64_t n = f->hdr_host->n_out;
    uint32_t fl = f->hdr_host->flags;
    if (n > max_out) { n = max_out; fl |= ADSB_FLAG_TRUNCATED; }
    if (n) {
        HIPCHK(hipMemcpyAsync(out, r.li.out, sizeof(adsb_frame) * n, hipMemcpyDeviceToHost, f->copy));
        HIPCHK(hipStreamSynchronize(f->copy));
    }
    *n_out = (size_t)n;
    if (flags) *flags = fl;
    return ADSB_OK;
}

// ---- measurement: the host-fed (PCIe-inclusive) rate of the streaming front end ---------------------------------------------
// What the reference's thread 1 -> thread 2 hand-over costs per buffer through adsb_feed_* (src/adsb.rs:75-89: playback
// sends 20 000-sample buffers; adsb.rs:59-64: MTU-sized reads), measured from C (no interpreter in the loop): a context
// and a feed of its own on `device`, synthetic samples written into the pinned ring by an in-place producer (acquire /
// push), two buffers in flight, every list popped; runs for about `seconds`.  bench.py reports it next to `value`
// (which is the HBM-resident rate and never includes PCIe).
extern "C" int adsb_measure_feed(int device, int sample_type, size_t chunk, double seconds, double *us_per_buffer,
                                 double *frames_per_buffer, uint64_t *buffers)
{
    if (!us_per_buffer || chunk < (size_t)kWindow || seconds <= 0 || (sample_type != ADSB_SAMPLE_I8 && sample_type != ADSB_SAMPLE_I16))
        return ADSB_E_ARG;
    const size_t bps = sample_type == ADSB_SAMPLE_I8 ? 2 : 4;
    adsb_synth_cfg sc;
    adsb_synth_default(&sc);
    sc.seed = 9;
    if (sample_type == ADSB_SAMPLE_I16) sc.amp_shift = 5;
    const int n_src = chunk <= (1u << 20) ? 8 : 2;
    std::vector<char> data(chunk * bps * n_src);
    int rc = adsb_synth_fill_host(&sc, sample_type, 0, 0, chunk * n_src, data.data());
    if (rc != ADSB_OK) return rc;
    adsb_cfg cfg{};
    cfg.abi_version = ADSB_ABI_VERSION;
    cfg.device = device;
    cfg.sample_type = sample_type;
    cfg.max_channels = 1;
    cfg.max_samples = chunk + kWindow;
    cfg.max_out = chunk / 200 + 4096;
    adsb_ctx *ctx = nullptr;
    if ((rc = adsb_create(&cfg, &ctx)) != ADSB_OK) return rc;
    adsb_feed_cfg fc{};
    fc.max_chunk = chunk;
    fc.carry = 0;
    fc.ring_slots = 3;
    adsb_feed *feed = nullptr;
    if ((rc = adsb_feed_open(ctx, &fc, &feed)) != ADSB_OK) { adsb_destroy(ctx); return rc; }
    std::vector<adsb_frame> frames(cfg.max_out);
    uint64_t total = 0, n_buf = 0;
    auto one = [&](uint64_t k, bool fill) {
        void *slot = nullptr;
        int r = adsb_feed_acquire(feed, &slot);
        // (a real producer -- SDR driver, file reader -- writes its samples straight into the slot: that is its cost, not
        // the hand-over's; the slots are filled during the warm-up rounds)
        if (r == ADSB_OK && fill) std::memcpy(slot, data.data() + (size_t)(k % n_src) * chunk * bps, chunk * bps);
        if (r == ADSB_OK) r = adsb_feed_push(feed, nullptr, chunk);
        if (r == ADSB_OK && adsb_feed_in_flight(feed) == 2) {
            size_t n = 0;
            r = adsb_feed_pop(feed, frames.data(), frames.size(), &n, nullptr, nullptr);
            total += n;
        }
        return r;
    };
    auto drain = [&]() {
        int r = ADSB_OK;
        while (r == ADSB_OK && adsb_feed_in_flight(feed) > 0) {
            size_t n = 0;
            r = adsb_feed_pop(feed, frames.data(), frames.size(), &n, nullptr, nullptr);
            total += n;
        }
        return r;
    };
    for (uint64_t k = 0; k < 6 && rc == ADSB_OK; ++k) rc = one(k, true);
    if (rc == ADSB_OK) rc = drain();
    total = 0;
    using clk = std::chrono::steady_clock;
    const auto t0 = clk::now();
    double dt = 0;
    while (rc == ADSB_OK) {
        for (int k = 0; k < 16 && rc == ADSB_OK; ++k, ++n_buf) rc = one(n_buf + 6, false);
        dt = std::chrono::duration<double>(clk::now() - t0).count();
        if (dt >= seconds) break;
    }
    if (rc == ADSB_OK) rc = drain();
    dt = std::chrono::duration<double>(clk::now() - t0).count();
    adsb_feed_close(feed);
    adsb_destroy(ctx);
    if (rc != ADSB_OK) return rc;
    *us_per_buffer = n_buf ? dt * 1e6 / (double)n_buf : 0.0;
    if (frames_per_buffer) *frames_per_buffer = n_buf ? (double)total / (double)n_buf : 0.0;
    if (buffers) *buffers = n_buf;
    return ADSB_OK;
}

// The box's pinned host -> device copy rate (one stream, `bytes` per copy): the ceiling of any host-fed path.
extern "C" int adsb_measure_pinned_copy(int device, size_t bytes, int iters, double *gbytes_per_s)
{
    if (!gbytes_per_s || bytes == 0 || iters <= 0) return ADSB_E_ARG;
    HIPCHK(hipSetDevice(device));
    void *h = nullptr, *d = nullptr;
    hipStream_t s = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipError_t e = hipHostMalloc(&h, bytes, hipHostMallocDefault);
    if (e == hipSuccess) e = hipMalloc(&d, bytes);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreate(&e0);
    if (e == hipSuccess) e = hipEventCreate(&e1);
    float ms = 0;
    if (e == hipSuccess) {
        std::memset(h, 1, bytes);
        e = hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, s); // warm-up
        if (e == hipSuccess) e = hipEventRecord(e0, s);
        for (int k = 0; k < iters && e == hipSuccess; ++k) e = hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipEventRecord(e1, s);
        if (e == hipSuccess) e = hipEventSynchronize(e1);
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (s) (void)hipStreamDestroy(s);
    (void)hipFree(d);
    if (h) (void)hipHostFree(h);
    if (e != hipSuccess) return (int)e;
    *gbytes_per_s = ms > 0 ? (double)bytes * iters / (ms * 1e-3) / 1e9 : 0.0;
    return ADSB_OK;
}
