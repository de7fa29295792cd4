// adsb_track_api.cpp -- the tracker's part of the extern "C" boundary (include/adsb_hip.h) over adsb_track.hip: the
// per-launch tracker (adsb_track_device), the persistent table (adsb_track_table_*) and the bank of tables
// (adsb_track_bank_*).  A table and a bank are one host-side store (TrackStore: a table is a store with one receiver),
// and every entry point below is its argument checks plus a call of a helper written once.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "adsb_fix.h"
#include "adsb_scratch.h"
#include "adsb_track_mlat.h"
#include "adsb_track_filter.h"
#include "adsb_track_modes.h"

using adsbk::TrackKind;
using adsbk::TrackRecord;

// What launch_track needs whatever the form: the list, u32 = 4 x [cap] (keys, vals, sorted keys, sorted vals)
static adsbk::TrackArgs track_args(TrackKind kind, const adsb_frame *frames, const adsb_packet_fields *fields, size_t n,
                                   double seconds_per_sample, uint32_t *u32, size_t cap, void *temp, size_t temp_bytes,
                                   adsb_track_point *points)
{
    adsbk::TrackArgs a{};
    a.kind = kind;
    a.frames = frames;
    a.fields = fields;
    a.n = (uint32_t)n;
    a.seconds_per_sample = seconds_per_sample;
    a.keys = u32;
    a.vals = u32 + cap;
    a.skeys = u32 + 2 * cap;
    a.svals = u32 + 3 * cap;
    a.temp = temp;
    a.temp_bytes = temp_bytes;
    a.points = points;
    return a;
}

extern "C" int adsb_track_device(adsb_ctx *c, double seconds_per_sample)
{
    if (!c || !(seconds_per_sample > 0.0)) return ADSB_E_ARG;
    if (!c->launched) return ADSB_E_STATE;
    if (c->launch().channels != 1) return ADSB_E_ARG;
    int rc = sync_header(c); // the list's length (and the rebuild after a slot-pool overflow)
    if (rc != ADSB_OK) return rc;
    if (!c->fields_current && (rc = adsb_decode_fields_device_async(c)) != ADSB_OK) return rc;
    HIPCHK(hipSetDevice(c->cfg.device));
    const size_t cap = (size_t)c->cfg.max_out;
    if (!c->trk_mem.p) {
        c->trk_temp_bytes = adsbk::track_sort_temp_bytes(cap);
        rc = carve_block(c, c->trk_mem, [&](Carve &k) {
            c->trk_u32 = k.take<uint32_t>(4 * cap);
            c->trk_temp = k.take<char>(c->trk_temp_bytes);
            c->trk_points = k.take<adsb_track_point>(cap);
            c->trk_aircraft = k.take<adsb_aircraft_record>(cap);
            c->trk_n_aircraft = k.take<uint64_t>(1);
        });
        if (rc != ADSB_OK) return rc;
    }
    const uint64_t n = std::min<uint64_t>(c->hdr_host->n_out, c->launch().cap);
    adsbk::TrackArgs a = track_args(TrackKind::kLaunch, c->launch().out, c->fields, n, seconds_per_sample, c->trk_u32, cap,
                                    c->trk_temp, c->trk_temp_bytes, c->trk_points);
    a.aircraft = c->trk_aircraft;
    a.max_aircraft = (uint32_t)cap;
    a.n_aircraft = c->trk_n_aircraft;
    HIPCHK(adsbk::launch_track(c->aux, a)); // same stream as the ordering pass and the field decode
    c->trk_n = (uint32_t)n;
    c->trk_done = true;
    return ADSB_OK;
}

extern "C" int adsb_fetch_track(adsb_ctx *c, adsb_track_point *points, size_t max_points, size_t *n_points,
                                adsb_aircraft_record *aircraft, size_t max_aircraft, size_t *n_aircraft)
{
    if (!c || (!points && max_points) || (!aircraft && max_aircraft)) return ADSB_E_ARG;
    if (!c->trk_done) return ADSB_E_STATE;
    HIPCHK(hipSetDevice(c->cfg.device));
    uint64_t na = 0;
    HIPCHK(hipMemcpyAsync(&na, c->trk_n_aircraft, sizeof(uint64_t), hipMemcpyDeviceToHost, c->aux));
    HIPCHK(hipStreamSynchronize(c->aux));
    const size_t np = std::min<size_t>(c->trk_n, max_points);
    const size_t nac = std::min<size_t>((size_t)na, max_aircraft);
    if (np) HIPCHK(hipMemcpyAsync(points, c->trk_points, sizeof(adsb_track_point) * np, hipMemcpyDeviceToHost, c->aux));
    if (nac) HIPCHK(hipMemcpyAsync(aircraft, c->trk_aircraft, sizeof(adsb_aircraft_record) * nac, hipMemcpyDeviceToHost, c->aux));
    HIPCHK(hipStreamSynchronize(c->aux));
    if (n_points) *n_points = np;
    if (n_aircraft) *n_aircraft = (size_t)na;
    return ADSB_OK;
}

// ---- the store behind adsb_track_table_* and adsb_track_bank_* -----------------------------------------------------
// Per-frame summaries and the changed list (adsb_track_*_summaries_reserve): everything here is carved by the
// reserve; `dev.out` null = no reserve.
struct TrackSummaries {
    adsbk::TrackSumDev dev{};
    TrackRecord *changed_rec = nullptr; // [changed_cap]: fetch_changed's device-side gather
    size_t changed_cap = 0;         // min(max_frames, record places): an update cannot touch more aircraft
    bool updated = false;           // an update ran since the reserve (and since the last reset)
    bool changed_valid = false;     // the last operation was an update: the changed list's slots still hold
};

// What a table and a bank share.  A table is a store with one receiver, found through dev.index; a bank finds its
// records through dev.hash and adds the receiver split's staging and the fused view (adsb_track_bank below).
struct TrackStore {
    adsb_ctx *ctx = nullptr;
    TrackKind kind = TrackKind::kTable;
    uint64_t max_frames = 0;
    double seconds_per_sample = 0.0;
    uint32_t n_receivers = 0, max_aircraft = 0; // max_aircraft: per receiver
    // One block of device memory per lifetime, carved into the arrays below (adsb_scratch.h): the store's own from
    // create to destroy, and one per reserve.  Every device pointer of the store points into one of them.
    DevBuf<char> mem, sum_mem, lvl_mem, fix_mem, mlat_mem, modes_mem, commb_mem, es_mem, filter_mem;
    adsbk::TrackStoreDev dev{};     // records [R x max_aircraft], slot [max_frames]; index [2^24] or hash, prefix, scan words
    uint32_t *words = nullptr;      // [3R]: size, flags, size_next (dev.size / dev.flags / dev.size_next)
    uint32_t *u32 = nullptr;        // 4 x [max_frames]: keys, vals, sorted keys, sorted vals
    void *temp = nullptr;
    size_t temp_bytes = 0;
    adsb_frame *frames = nullptr;   // [max_frames]: device copy of a host list
    adsb_frame *pinned = nullptr;   // [max_frames]: pinned staging of that copy
    hipEvent_t copied = nullptr;    // the last copies out of the pinned staging (a bank: and meta_pinned) have finished
    adsb_packet_fields *fields = nullptr; // [max_frames]
    adsb_track_point *points = nullptr;   // [max_frames], the last update's, list order
    uint32_t *exp_u32 = nullptr;    // 2 x [R x max_aircraft]: expire's keep flags and their scan
    void *exp_temp = nullptr;       // expire's scan
    size_t exp_temp_bytes = 0;
    uint64_t *meta = nullptr;       // a bank's, device [2R + 1]: prefix of the host counts [R + 1], then sample_base [R]
    uint64_t *meta_pinned = nullptr; // pinned staging of meta
    uint32_t n_points = 0;
    bool updated = false;
    TrackSummaries sum;
    // per-aircraft levels (adsb_track_*_levels_reserve): all of it made by the reserve; dev.lvl null = no reserve
    adsbk::TrackLvlDev lvl{};
    adsb_frame_level *lvl_frames = nullptr; // [max_frames]: device copy of a host levels array
    adsb_frame_level *lvl_pinned = nullptr; // [max_frames]: pinned staging of that copy (s.copied covers it too)
    // positions from single messages (adsb_track_*_fixes_reserve): all of it carved by the reserve; dev.fix null = none
    adsbk::TrackFixDev fix{};
    // multilaterated positions per aircraft (adsb_track_table_mlat_reserve): all of it made by the reserve; dev.mlat null
    // = none
    adsbk::TrackMlatDev mlat{};
    adsb_mlat_fix *mlat_fixes = nullptr;  // [max_frames]: device copy of a host fixes array
    adsb_mlat_fix *mlat_pinned = nullptr; // [max_frames]: pinned staging of that copy (s.copied covers it too)
    uint32_t mlat_n = 0;                  // frames of the last update_mlat
    bool mlat_updated = false;            // an update_mlat ran since the reserve (and since the last reset)
    // filtered mlat track per aircraft (adsb_track_table_filter_reserve): all of it carved by the reserve; dev.filter
    // null = none.  Its per-frame arrays speak of the list mlat_n counts.
    adsbk::TrackFilterDev filter{};
    bool filter_updated = false;          // an update given fixes ran since the reserve (and since the last reset)
    // Mode S replies per aircraft (adsb_track_table_modes_reserve): all of it made by the reserve; dev.modes null = none
    adsbk::TrackModesDev modes{};
    adsb_modes_rec *modes_recs = nullptr;   // [max_frames]: device copy of a host recs array
    adsb_modes_rec *modes_pinned = nullptr; // [max_frames]: pinned staging of that copy (s.copied covers it too)
    // Comm-B registers per aircraft (adsb_track_table_commb_reserve): all of it made by the reserve; dev.commb null = none
    adsbk::TrackCommbDev commb{};
    adsb_commb_rec *commb_recs = nullptr;   // [max_frames]: device copy of a host commb array
    adsb_commb_rec *commb_pinned = nullptr; // [max_frames]: pinned staging of that copy (s.copied covers it too)
    uint32_t commb_n = 0;                   // frames of the last update_commb
    bool commb_updated = false;             // an update_commb ran since the reserve (and since the last reset)
    // Extended squitter status per aircraft (adsb_track_table_es_reserve): all of it made by the reserve; dev.es null = none
    adsbk::TrackEsDev es{};
    adsb_es_rec *es_recs = nullptr;         // [max_frames]: device copy of a host es array
    adsb_es_rec *es_pinned = nullptr;       // [max_frames]: pinned staging of that copy (s.copied covers it too)
    uint32_t es_n = 0;                      // frames of the last update_es
    bool es_updated = false;                // an update_es ran since the reserve (and since the last reset)

    size_t places() const { return (size_t)n_receivers * max_aircraft; }
};

struct adsb_track_table : TrackStore {};

struct adsb_track_bank : TrackStore {
    // the fused view (adsb_track_bank_fuse_*): all of it made by fuse_reserve, nothing before
    DevBuf<char> fuse_mem;          // one block, carved into the arrays of `fuse`
    DevBuf<adsb_fused_level> fuse_lvl_out; // [fuse.max]: only with a levels reserve too (the second reserve makes it)
    struct Fuse {
        void *keys = nullptr;       // 2 x [places] sort keys (uint32_t, uint64_t above kFuseWideReceivers): in, sorted
        uint32_t *vals = nullptr;   // 2 x [places]: places in, sorted
        uint32_t *start = nullptr;  // [max]
        adsb_fused_aircraft *out = nullptr; // [max]
        uint64_t *counts = nullptr; // device [3]: records written, distinct ICAOs, ADSB_TRACK_FUSED_TRUNCATED
        void *temp = nullptr;
        size_t temp_bytes = 0;
        size_t max = 0;             // 0: no reserve
        uint32_t lanes = 0;
        bool fused = false;         // a fuse ran since the last reserve
        bool fused_levels = false;  // ... and also computed fuse_lvl_out
    } fuse;
};

// The three pinned staging buffers (frames, level records, a bank's meta) are host memory, not device scratch
template <class T>
static bool pinned_make(T *&p, size_t n)
{
    return hipHostMalloc((void **)&p, sizeof(T) * n, hipHostMallocDefault) == hipSuccess;
}

template <class T>
static void pinned_free(T *&p)
{
    if (p) (void)hipHostFree(p);
    p = nullptr;
}

// The levels reserve undone.  Nothing on the device uses it any more (its clear has been waited for, or never ran).
static void store_levels_drop(TrackStore &s)
{
    drop(s.lvl_mem);
    pinned_free(s.lvl_pinned);
    s.dev.lvl = nullptr;
    s.lvl = {};
    s.lvl_frames = nullptr;
}

// The fixes reserve undone, under the same condition.
static void store_fixes_drop(TrackStore &s)
{
    drop(s.fix_mem);
    s.dev.fix = nullptr;
    s.dev.site = nullptr;
    s.fix = {};
}

// The mlat reserve undone, under the same condition.
static void store_mlat_drop(TrackStore &s)
{
    drop(s.mlat_mem);
    pinned_free(s.mlat_pinned);
    s.dev.mlat = nullptr;
    s.mlat = {};
    s.mlat_fixes = nullptr;
}

// The filter reserve undone, under the same condition.
static void store_filter_drop(TrackStore &s)
{
    drop(s.filter_mem);
    s.dev.filter = nullptr;
    s.filter = {};
}

// The list fetch_frame_mlat (and, with a filter reserve, fetch_frame_filter) speaks of: n frames
static void store_mlat_list(TrackStore &s, size_t n)
{
    s.mlat_n = (uint32_t)n;
    s.mlat_updated = true;
    if (s.dev.filter) s.filter_updated = true;
}

// The modes reserve undone, under the same condition.
static void store_modes_drop(TrackStore &s)
{
    drop(s.modes_mem);
    pinned_free(s.modes_pinned);
    s.dev.modes = nullptr;
    s.modes = {};
    s.modes_recs = nullptr;
}

// The commb reserve undone, under the same condition.
static void store_commb_drop(TrackStore &s)
{
    drop(s.commb_mem);
    pinned_free(s.commb_pinned);
    s.dev.commb = nullptr;
    s.commb = {};
    s.commb_recs = nullptr;
}

// The es reserve undone, under the same condition.
static void store_es_drop(TrackStore &s)
{
    drop(s.es_mem);
    pinned_free(s.es_pinned);
    s.dev.es = nullptr;
    s.es = {};
    s.es_recs = nullptr;
}

// Sizes, and the store's own block: what a table and a bank share, then what each kind adds (a bank has set
// dev.hash_mask).  false: an allocation failed (the caller releases what was made)
static bool store_alloc(TrackStore &s, adsb_ctx *c, TrackKind kind, uint32_t n_receivers, uint32_t max_aircraft, uint64_t max_frames,
                        double seconds_per_sample, size_t temp_bytes)
{
    s.ctx = c;
    s.kind = kind;
    s.max_frames = max_frames;
    s.seconds_per_sample = seconds_per_sample;
    s.dev.n_receivers = s.n_receivers = n_receivers;
    s.dev.max_aircraft = s.max_aircraft = max_aircraft;
    s.temp_bytes = temp_bytes;
    s.exp_temp_bytes = adsbk::track_expire_temp_bytes(s.places());
    const size_t nf = (size_t)max_frames, nr = n_receivers;
    const int rc = carve_block(c, s.mem, [&](Carve &k) {
        s.dev.rec = k.take<TrackRecord>(s.places());
        s.words = k.take<uint32_t>(3 * nr);
        s.dev.size = s.words;
        s.dev.flags = s.words + nr;
        s.dev.size_next = s.words + 2 * nr;
        s.dev.slot = k.take<uint32_t>(nf);
        s.u32 = k.take<uint32_t>(4 * nf);
        s.temp = k.take<char>(s.temp_bytes);
        s.frames = k.take<adsb_frame>(nf);
        s.fields = k.take<adsb_packet_fields>(nf);
        s.points = k.take<adsb_track_point>(nf);
        s.exp_u32 = k.take<uint32_t>(2 * s.places());
        s.exp_temp = k.take<char>(s.exp_temp_bytes);
        if (kind == TrackKind::kTable) {
            s.dev.index = k.take<uint32_t>((size_t)1 << 24);
        } else {
            s.dev.hash = k.take<unsigned long long>(s.dev.hash_mask + 1);
            s.dev.prefix = k.take<uint32_t>(nr + 1);
            s.meta = k.take<uint64_t>(2 * nr + 1);
            s.dev.sample_base = s.meta + nr + 1;
            s.dev.mark = k.take<unsigned long long>(nf);
            s.dev.excl = k.take<unsigned long long>(nf);
            s.dev.seg_slot = k.take<uint32_t>(nf);
        }
    });
    return rc == ADSB_OK && pinned_make(s.pinned, nf) &&
           (kind == TrackKind::kTable || pinned_make(s.meta_pinned, 2 * nr + 1)) &&
           hipEventCreateWithFlags(&s.copied, hipEventDisableTiming) == hipSuccess;
}

// Waits for the stream, then frees whatever of the store exists
static void store_release(TrackStore &s)
{
    (void)hipSetDevice(s.ctx->cfg.device);
    (void)hipStreamSynchronize(s.ctx->aux);
    drop(s.mem);
    drop(s.sum_mem);
    drop(s.lvl_mem);
    drop(s.fix_mem);
    drop(s.mlat_mem);
    store_modes_drop(s);
    store_commb_drop(s);
    store_es_drop(s);
    drop(s.filter_mem);
    pinned_free(s.pinned);
    pinned_free(s.lvl_pinned);
    pinned_free(s.mlat_pinned);
    pinned_free(s.meta_pinned);
    if (s.copied) (void)hipEventDestroy(s.copied);
}

static int store_reset(TrackStore *s)
{
    if (!s) return ADSB_E_ARG;
    HIPCHK(hipSetDevice(s->ctx->cfg.device));
    if (s->kind == TrackKind::kTable)
        HIPCHK(hipMemsetAsync(s->dev.index, 0, sizeof(uint32_t) << 24, s->ctx->aux));
    else
        HIPCHK(hipMemsetAsync(s->dev.hash, 0, sizeof(unsigned long long) * (s->dev.hash_mask + 1), s->ctx->aux));
    HIPCHK(hipMemsetAsync(s->words, 0, sizeof(uint32_t) * 3 * s->n_receivers, s->ctx->aux));
    if (s->dev.fix) HIPCHK(adsbk::launch_track_fixes_clear(s->ctx->aux, s->dev.fix, s->places()));
    if (s->dev.mlat) HIPCHK(adsbk::launch_track_mlat_clear(s->ctx->aux, s->dev.mlat, s->places()));
    if (s->dev.modes) HIPCHK(adsbk::launch_track_modes_clear(s->ctx->aux, s->dev.modes, s->places()));
    if (s->dev.commb) HIPCHK(adsbk::launch_track_commb_clear(s->ctx->aux, s->dev.commb, s->places()));
    s->mlat_updated = false;
    if (s->dev.filter) HIPCHK(adsbk::launch_track_filter_clear(s->ctx->aux, s->dev.filter, s->places()));
    s->filter_updated = false;
    if (s->dev.es) HIPCHK(adsbk::launch_track_es_clear(s->ctx->aux, s->dev.es, s->places()));
    s->commb_updated = false;
    s->es_updated = false;
    s->n_points = 0;
    s->updated = false;
    s->sum.updated = s->sum.changed_valid = false;
    return ADSB_OK;
}

// The end of a create: the first reset and a wait for it; a store that could not be completed is destroyed
template <class S>
static int store_created(S *s, bool allocated, void (*destroy)(S *), S **out)
{
    int rc = allocated ? store_reset(s) : ADSB_E_NOMEM;
    if (rc == ADSB_OK && hipStreamSynchronize(s->ctx->aux) != hipSuccess) rc = ADSB_E_NOMEM;
    if (rc != ADSB_OK) {
        (void)hipGetLastError();
        destroy(s);
        return rc;
    }
    *out = s;
    return ADSB_OK;
}

// Host frames through the pinned staging, so the caller's array is free when the update returns.  The caller has waited
// for s.copied before (the previous update's copy out of the staging has finished) and records it after.
static int store_stage_frames(TrackStore &s, const adsb_frame *host, size_t n)
{
    std::memcpy(s.pinned, host, sizeof(adsb_frame) * n);
    HIPCHK(hipMemcpyAsync(s.frames, s.pinned, sizeof(adsb_frame) * n, hipMemcpyHostToDevice, s.ctx->aux));
    return ADSB_OK;
}

// The same for a host levels array (the *_update_levels forms), under the same event
static int store_stage_levels(TrackStore &s, const adsb_frame_level *host, size_t n)
{
    std::memcpy(s.lvl_pinned, host, sizeof(adsb_frame_level) * n);
    HIPCHK(hipMemcpyAsync(s.lvl_frames, s.lvl_pinned, sizeof(adsb_frame_level) * n, hipMemcpyHostToDevice, s.ctx->aux));
    return ADSB_OK;
}

// The same for a host fixes array (update_mlat), under the same event
static int store_stage_mlat(TrackStore &s, const adsb_mlat_fix *host, size_t n)
{
    std::memcpy(s.mlat_pinned, host, sizeof(adsb_mlat_fix) * n);
    HIPCHK(hipMemcpyAsync(s.mlat_fixes, s.mlat_pinned, sizeof(adsb_mlat_fix) * n, hipMemcpyHostToDevice, s.ctx->aux));
    return ADSB_OK;
}

// The same for a host recs array (update_modes), under the same event
static int store_stage_modes(TrackStore &s, const adsb_modes_rec *host, size_t n)
{
    std::memcpy(s.modes_pinned, host, sizeof(adsb_modes_rec) * n);
    HIPCHK(hipMemcpyAsync(s.modes_recs, s.modes_pinned, sizeof(adsb_modes_rec) * n, hipMemcpyHostToDevice, s.ctx->aux));
    return ADSB_OK;
}

// The same for a host commb array (update_commb), under the same event
static int store_stage_commb(TrackStore &s, const adsb_commb_rec *host, size_t n)
{
    std::memcpy(s.commb_pinned, host, sizeof(adsb_commb_rec) * n);
    HIPCHK(hipMemcpyAsync(s.commb_recs, s.commb_pinned, sizeof(adsb_commb_rec) * n, hipMemcpyHostToDevice, s.ctx->aux));
    return ADSB_OK;
}

// The same for a host es array (update_es), under the same event
static int store_stage_es(TrackStore &s, const adsb_es_rec *host, size_t n)
{
    std::memcpy(s.es_pinned, host, sizeof(adsb_es_rec) * n);
    HIPCHK(hipMemcpyAsync(s.es_recs, s.es_pinned, sizeof(adsb_es_rec) * n, hipMemcpyHostToDevice, s.ctx->aux));
    return ADSB_OK;
}

// The bookkeeping every update starts with (an empty one too: no summaries, an empty changed list); false: n == 0,
// nothing to launch
static bool store_begin_update(TrackStore &s, size_t n)
{
    s.n_points = (uint32_t)n;
    s.updated = true;
    if (s.sum.dev.out) s.sum.updated = s.sum.changed_valid = true;
    return n != 0;
}

// Enqueues field decode and the tracker kernels over n frames at `list` (device), after the ctx's ordering pass and
// field decode (same stream); dev: s.dev, or a bank's copy of it with this update's receiver split; levels (device,
// or null): also the level merge; mlat_fixes (device, or null): also the mlat merge; recs (device, or null): the list is
// keyed by the records' addresses and the modes merge runs too (update_modes), with the modes reserve's scratch, which
// holds the 25-bit sort; commb (device, or null; only with recs): the commb step runs too (update_commb); es (device,
// or null): the es step runs too (update_es)
static int store_run(TrackStore &s, const adsb_frame *list, size_t n, uint64_t sample_base,
                     const adsbk::TrackStoreDev &dev, const adsb_frame_level *levels = nullptr,
                     const adsb_mlat_fix *mlat_fixes = nullptr, const adsb_modes_rec *recs = nullptr,
                     const adsb_commb_rec *commb = nullptr, const adsb_es_rec *es = nullptr)
{
    HIPCHK(adsbk::launch_decode_fields(s.ctx->aux, list, nullptr, (uint32_t)n, s.fields));
    adsbk::TrackArgs a = track_args(s.kind, list, s.fields, n, s.seconds_per_sample, s.u32, (size_t)s.max_frames,
                                    s.temp, s.temp_bytes, s.points);
    a.sample_base = sample_base;
    a.store = &dev;
    a.sum = s.sum.dev.out ? &s.sum.dev : nullptr;
    a.levels = levels;
    a.lvl = levels ? &s.lvl : nullptr;
    a.fix = dev.fix ? &s.fix : nullptr;
    a.mlat_fixes = mlat_fixes;
    a.mlat = mlat_fixes ? &s.mlat : nullptr;
    a.filter = mlat_fixes && dev.filter ? &s.filter : nullptr;
    if (recs) {
        a.modes_recs = recs;
        a.modes = &s.modes;
        a.modes_fields = s.fields;
        a.temp = s.modes.temp;
        a.temp_bytes = s.modes.temp_bytes;
        if (commb) {
            a.commb_recs = commb;
            a.commb = &s.commb;
        }
    }
    if (es) {
        a.es_recs = es;
        a.es = &s.es;
    }
    HIPCHK(adsbk::launch_track(s.ctx->aux, a));
    return ADSB_OK;
}

// The store's device arrays a caller may fetch or borrow; null: not reserved, or (the per-frame ones, which hold the
// last update's list) no update yet.
static const adsb_track_point *points_of(TrackStore &s) { return s.updated ? s.points : nullptr; }
static const adsb_aircraft_record *summaries_of(TrackStore &s) { return s.sum.updated ? s.sum.dev.out : nullptr; }
static const adsb_frame_fix *frame_fixes_of(TrackStore &s) { return s.dev.fix && s.updated ? s.fix.out : nullptr; }
static const adsb_aircraft_level *levels_of(TrackStore &s) { return s.dev.lvl; }
static const adsb_fix *fixes_of(TrackStore &s) { return s.dev.fix; }
static const adsb_aircraft_mlat *mlat_of(TrackStore &s) { return s.dev.mlat; }
static const adsb_aircraft_filter *filter_of(TrackStore &s) { return s.dev.filter; }
static const adsb_aircraft_modes *modes_of(TrackStore &s) { return s.dev.modes; }
static const adsb_aircraft_commb *commb_of(TrackStore &s) { return s.dev.commb; }
static const adsb_aircraft_es *es_of(TrackStore &s) { return s.dev.es; }

template <class T>
static int store_device(TrackStore *s, const T *of(TrackStore &), const T **dev)
{
    if (!s) return ADSB_E_ARG;
    const T *p = of(*s);
    if (!p) return ADSB_E_STATE;
    if (dev) *dev = p;
    return ADSB_OK;
}

// Waits.  The first min(list, max) per-frame records of the last update, list order; *n = how many were copied, or the
// list's length.
enum class Report { kCopied, kListLength };
template <class T>
static int store_fetch_frames(TrackStore *s, const T *of(TrackStore &), T *out, size_t max, size_t *n, Report report)
{
    if (!s || (!out && max)) return ADSB_E_ARG;
    const T *src = of(*s);
    if (!src) return ADSB_E_STATE;
    HIPCHK(hipSetDevice(s->ctx->cfg.device));
    const size_t take = std::min<size_t>(s->n_points, max);
    if (take) HIPCHK(hipMemcpyAsync(out, src, sizeof(T) * take, hipMemcpyDeviceToHost, s->ctx->aux));
    HIPCHK(hipStreamSynchronize(s->ctx->aux));
    if (n) *n = report == Report::kCopied ? take : s->n_points;
    return ADSB_OK;
}

// Records of one receiver (slots in admission order) as fetch returns them: ascending ICAO.
static void sort_by_icao(std::vector<TrackRecord> &recs)
{
    std::sort(recs.begin(), recs.end(), [](const TrackRecord &x, const TrackRecord &y) { return x.a.icao < y.a.icao; });
}

// Waits.  Receiver by receiver: its records (slots are in admission order) sorted by ICAO, out[k] = get(record) for
// the first `max` records in all and nothing past them; *n = records held in all, counts[r] = records COPIED for
// receiver r, flags[r] = its device flags word (each optional).
template <class T, class Get>
static int store_fetch(TrackStore *s, T *out, size_t max, size_t *n, uint64_t *counts, uint32_t *flags, Get get)
{
    if (!s || (!out && max)) return ADSB_E_ARG;
    adsb_ctx *c = s->ctx;
    HIPCHK(hipSetDevice(c->cfg.device));
    const uint32_t nr = s->n_receivers;
    std::vector<uint32_t> w(2 * (size_t)nr); // sizes, then flags
    HIPCHK(hipMemcpyAsync(w.data(), s->words, sizeof(uint32_t) * w.size(), hipMemcpyDeviceToHost, c->aux));
    HIPCHK(hipStreamSynchronize(c->aux));
    size_t total = 0, copied = 0;
    std::vector<TrackRecord> recs;
    for (uint32_t r = 0; r < nr; ++r) {
        const size_t size = std::min<uint32_t>(w[r], s->max_aircraft);
        total += size;
        const size_t take = std::min(size, max - copied);
        if (take) {
            recs.resize(size);
            HIPCHK(hipMemcpyAsync(recs.data(), s->dev.rec + (size_t)r * s->max_aircraft, sizeof(TrackRecord) * size,
                                  hipMemcpyDeviceToHost, c->aux));
            HIPCHK(hipStreamSynchronize(c->aux));
            sort_by_icao(recs);
            for (size_t k = 0; k < take; ++k) out[copied + k] = get(recs[k]);
        }
        copied += take;
        if (counts) counts[r] = take;
        if (flags) flags[r] = w[nr + r];
    }
    if (n) *n = total;
    return ADSB_OK;
}

static adsb_aircraft_record record_of(const TrackRecord &r) { return r.a; }
static double last_heard_of(const TrackRecord &r) { return r.last_heard; }
static adsb_velocity velocity_of(const TrackRecord &r) { return r.vel; }

// before: [n_receivers] cuts
static int store_expire(TrackStore *s, const double *before)
{
    if (!s || !before) return ADSB_E_ARG;
    adsbk::ExpireArgs a{};
    for (uint32_t r = 0; r < s->n_receivers; ++r) { // n_receivers <= kMaxReceivers (create checks)
        if (std::isnan(before[r])) return ADSB_E_ARG;
        a.cut.before[r] = before[r];                 // by value in the kernel's arguments: no staging, no wait
    }
    HIPCHK(hipSetDevice(s->ctx->cfg.device));
    a.kind = s->kind;
    a.store = &s->dev;
    a.keep = s->exp_u32;
    a.rank = s->exp_u32 + s->places();
    a.temp = s->exp_temp;
    a.temp_bytes = s->exp_temp_bytes;
    HIPCHK(adsbk::launch_track_expire(s->ctx->aux, a)); // after the store's last update (same stream)
    s->sum.changed_valid = false; // slots move
    return ADSB_OK;
}

// A second reserve keeps what the first one made
static int store_summaries_reserve(TrackStore *st)
{
    if (!st) return ADSB_E_ARG;
    HIPCHK(hipSetDevice(st->ctx->cfg.device));
    TrackSummaries &s = st->sum;
    if (s.dev.out) return ADSB_OK;
    const size_t max_frames = (size_t)st->max_frames;
    s.changed_cap = std::min(max_frames, st->places());
    s.dev.temp_bytes = adsbk::track_summaries_temp_bytes(max_frames);
    const int rc = carve_block(st->ctx, st->sum_mem, [&](Carve &k) {
        s.dev.scan = k.take<adsbk::TrackSumTuple>(max_frames);
        s.dev.changed = k.take<uint32_t>(max_frames);
        s.dev.n_changed = k.take<uint32_t>(1);
        s.dev.temp = k.take<char>(s.dev.temp_bytes);
        s.changed_rec = k.take<TrackRecord>(s.changed_cap);
        s.dev.out = k.take<adsb_aircraft_record>(max_frames);
    });
    if (rc != ADSB_OK) s = {};
    return rc;
}

// Waits; gathers the changed list's records on the device and copies only them.  counts (optional, [n_receivers]): how
// many of the records returned belong to each receiver (slot / max_aircraft).
static int store_fetch_changed(TrackStore *st, adsb_aircraft_record *out, double *last_heard, adsb_velocity *velocity,
                               size_t max, size_t *n, uint64_t *counts)
{
    if (!st) return ADSB_E_ARG;
    TrackSummaries &s = st->sum;
    adsb_ctx *c = st->ctx;
    if (!s.dev.out || !s.updated || !s.changed_valid) return ADSB_E_STATE;
    HIPCHK(hipSetDevice(c->cfg.device));
    if (counts) std::fill(counts, counts + st->n_receivers, (uint64_t)0);
    uint32_t nc = 0;
    if (st->n_points) { // an empty update launched nothing: its list is empty, and the device word is an older update's
        const uint32_t most = (uint32_t)std::min(std::min<size_t>(st->n_points, s.changed_cap), max);
        HIPCHK(adsbk::launch_track_changed(c->aux, st->dev.rec, s.dev, most, s.changed_rec));
        HIPCHK(hipMemcpyAsync(&nc, s.dev.n_changed, sizeof(nc), hipMemcpyDeviceToHost, c->aux));
        HIPCHK(hipStreamSynchronize(c->aux));
        const size_t take = std::min<size_t>(nc, most);
        if (take) {
            std::vector<TrackRecord> recs(take);
            std::vector<uint32_t> slots(take);
            HIPCHK(hipMemcpyAsync(recs.data(), s.changed_rec, sizeof(TrackRecord) * take, hipMemcpyDeviceToHost, c->aux));
            HIPCHK(hipMemcpyAsync(slots.data(), s.dev.changed, sizeof(uint32_t) * take, hipMemcpyDeviceToHost, c->aux));
            HIPCHK(hipStreamSynchronize(c->aux));
            for (size_t k = 0; k < take; ++k) {
                if (out) out[k] = recs[k].a;
                if (last_heard) last_heard[k] = recs[k].last_heard;
                if (velocity) velocity[k] = recs[k].vel;
                if (counts) ++counts[slots[k] / st->max_aircraft]; // a slot = receiver x max_aircraft + place
            }
        }
    }
    if (n) *n = nc;
    return ADSB_OK;
}

// Waits for the device (the clear); a second reserve keeps what the first one made
static int store_levels_reserve(TrackStore *st)
{
    if (!st) return ADSB_E_ARG;
    HIPCHK(hipSetDevice(st->ctx->cfg.device));
    if (st->dev.lvl) return ADSB_OK;
    const size_t nf = (size_t)st->max_frames;
    st->lvl.temp_bytes = adsbk::track_levels_temp_bytes(nf);
    const int rc = carve_block(st->ctx, st->lvl_mem, [&](Carve &k) {
        st->dev.lvl = k.take<adsb_aircraft_level>(st->places());
        st->lvl.scan = k.take<adsbk::TrackLvlTuple>(nf);
        st->lvl.temp = k.take<char>(st->lvl.temp_bytes);
        st->lvl_frames = k.take<adsb_frame_level>(nf);
    });
    if (rc != ADSB_OK || !pinned_make(st->lvl_pinned, nf) ||
        adsbk::launch_track_levels_clear(st->ctx->aux, st->dev.lvl, st->places()) != hipSuccess ||
        hipStreamSynchronize(st->ctx->aux) != hipSuccess) {
        (void)hipGetLastError();
        store_levels_drop(*st);
        return ADSB_E_NOMEM;
    }
    return ADSB_OK;
}

// Waits.  As store_fetch, receiver by receiver in ascending ICAO: the side record (a level record, a fix) beside each
// record; side: the store's device array of them, one per place.
template <class T>
static int store_fetch_side(TrackStore *s, const T *side_of(TrackStore &), T *out, size_t max, size_t *n)
{
    if (!s || (!out && max)) return ADSB_E_ARG;
    const T *side = side_of(*s);
    if (!side) return ADSB_E_STATE;
    adsb_ctx *c = s->ctx;
    HIPCHK(hipSetDevice(c->cfg.device));
    const uint32_t nr = s->n_receivers;
    std::vector<uint32_t> w(nr); // sizes
    HIPCHK(hipMemcpyAsync(w.data(), s->words, sizeof(uint32_t) * w.size(), hipMemcpyDeviceToHost, c->aux));
    HIPCHK(hipStreamSynchronize(c->aux));
    size_t total = 0, copied = 0;
    std::vector<TrackRecord> recs;
    std::vector<T> lv;
    std::vector<uint32_t> order;
    for (uint32_t r = 0; r < nr; ++r) {
        const size_t size = std::min<uint32_t>(w[r], s->max_aircraft);
        total += size;
        const size_t take = std::min(size, max - copied);
        if (take) {
            recs.resize(size);
            lv.resize(size);
            order.resize(size);
            HIPCHK(hipMemcpyAsync(recs.data(), s->dev.rec + (size_t)r * s->max_aircraft, sizeof(TrackRecord) * size,
                                  hipMemcpyDeviceToHost, c->aux));
            HIPCHK(hipMemcpyAsync((void *)lv.data(), side + (size_t)r * s->max_aircraft, sizeof(T) * size,
                                  hipMemcpyDeviceToHost, c->aux));
            HIPCHK(hipStreamSynchronize(c->aux));
            for (size_t k = 0; k < size; ++k) order[k] = (uint32_t)k;
            std::sort(order.begin(), order.end(),
                      [&](uint32_t x, uint32_t y) { return recs[x].a.icao < recs[y].a.icao; }); // distinct per receiver
            for (size_t k = 0; k < take; ++k) out[copied + k] = lv[order[k]];
        }
        copied += take;
    }
    if (n) *n = total;
    return ADSB_OK;
}

// ---- positions from single messages -----------------------------------------------------------------------------------
// sites: [n_receivers], checked by the caller.  Waits for the device (the sizes, the clear).
static int store_fixes_reserve(TrackStore *st, const adsb_site *sites)
{
    adsb_ctx *c = st->ctx;
    HIPCHK(hipSetDevice(c->cfg.device));
    const uint32_t nr = st->n_receivers;
    std::vector<uint32_t> sizes(nr);
    HIPCHK(hipMemcpyAsync(sizes.data(), st->words, sizeof(uint32_t) * nr, hipMemcpyDeviceToHost, c->aux));
    HIPCHK(hipStreamSynchronize(c->aux));
    for (uint32_t r = 0; r < nr; ++r)
        if (sizes[r] != 0) return ADSB_E_STATE; // its aircraft's fixes would miss the frames heard so far
    if (!st->dev.fix) {
        const size_t nf = (size_t)st->max_frames;
        st->fix.temp_bytes = adsbk::track_fixes_temp_bytes(nf);
        const int rc = carve_block(c, st->fix_mem, [&](Carve &k) {
            st->dev.fix = k.take<adsb_fix>(st->places());
            st->dev.site = k.take<adsb_site>(nr);
            st->fix.out = k.take<adsb_frame_fix>(nf);
            st->fix.rem = k.take<adsbk::FixRem>(nf);
            st->fix.scan = k.take<adsbk::TrackFixTuple>(nf);
            st->fix.temp = k.take<char>(st->fix.temp_bytes);
        });
        if (rc != ADSB_OK || adsbk::launch_track_fixes_clear(c->aux, st->dev.fix, st->places()) != hipSuccess ||
            hipStreamSynchronize(c->aux) != hipSuccess) {
            (void)hipGetLastError();
            store_fixes_drop(*st);
            return ADSB_E_NOMEM;
        }
    }
    // the stream is idle: a plain copy from the caller's array
    HIPCHK(hipMemcpy((void *)st->dev.site, sites, sizeof(adsb_site) * nr, hipMemcpyHostToDevice));
    return ADSB_OK;
}

// ---- multilaterated positions per aircraft ----------------------------------------------------------------------------
// Waits for the device (the clear); a second reserve keeps what the first one made, its limit too
static int store_mlat_reserve(TrackStore *st, double max_disagreement_m)
{
    HIPCHK(hipSetDevice(st->ctx->cfg.device));
    if (st->dev.mlat) return ADSB_OK;
    const size_t nf = (size_t)st->max_frames;
    st->mlat.temp_bytes = adsbk::track_mlat_temp_bytes(nf);
    st->mlat.max_disagreement_m = max_disagreement_m;
    const int rc = carve_block(st->ctx, st->mlat_mem, [&](Carve &k) {
        st->dev.mlat = k.take<adsb_aircraft_mlat>(st->places());
        st->mlat.out = k.take<adsb_frame_mlat>(nf);
        st->mlat.in = k.take<adsbk::TrackMlatTuple>(nf);
        st->mlat.scan = k.take<adsbk::TrackMlatTuple>(nf);
        st->mlat.temp = k.take<char>(st->mlat.temp_bytes);
        st->mlat_fixes = k.take<adsb_mlat_fix>(nf);
    });
    if (rc != ADSB_OK || !pinned_make(st->mlat_pinned, nf) ||
        adsbk::launch_track_mlat_clear(st->ctx->aux, st->dev.mlat, st->places()) != hipSuccess ||
        hipStreamSynchronize(st->ctx->aux) != hipSuccess) {
        (void)hipGetLastError();
        store_mlat_drop(*st);
        return ADSB_E_NOMEM;
    }
    return ADSB_OK;
}

// ---- filtered mlat track per aircraft --------------------------------------------------------------------------------
// Waits for the device (the clear); a second reserve keeps what the first one made, its cfg too.  cfg: resolved.
static int store_filter_reserve(TrackStore *st, const adsb_track_filter_cfg &cfg)
{
    HIPCHK(hipSetDevice(st->ctx->cfg.device));
    if (!st->dev.mlat) return ADSB_E_STATE;
    if (st->dev.filter) return ADSB_OK;
    const size_t nf = (size_t)st->max_frames;
    st->filter.cfg = cfg;
    const int rc = carve_block(st->ctx, st->filter_mem, [&](Carve &k) {
        st->dev.filter = k.take<adsb_aircraft_filter>(st->places());
        st->filter.op = k.take<adsb_filter_operand>(nf);
        st->filter.out = k.take<adsb_frame_filter>(nf);
    });
    if (rc != ADSB_OK || adsbk::launch_track_filter_clear(st->ctx->aux, st->dev.filter, st->places()) != hipSuccess ||
        hipStreamSynchronize(st->ctx->aux) != hipSuccess) {
        (void)hipGetLastError();
        store_filter_drop(*st);
        return ADSB_E_NOMEM;
    }
    st->filter_updated = false;
    return ADSB_OK;
}

// ---- Mode S replies per aircraft --------------------------------------------------------------------------------------
// Waits for the device (the clear); a second reserve keeps what the first one made
static int store_modes_reserve(TrackStore *st)
{
    HIPCHK(hipSetDevice(st->ctx->cfg.device));
    if (st->dev.modes) return ADSB_OK;
    const size_t nf = (size_t)st->max_frames;
    st->modes.temp_bytes = adsbk::track_modes_temp_bytes(nf);
    const int rc = carve_block(st->ctx, st->modes_mem, [&](Carve &k) {
        st->dev.modes = k.take<adsb_aircraft_modes>(st->places());
        st->modes.in = k.take<adsbk::TrackModesTuple>(nf);
        st->modes.scan = k.take<adsbk::TrackModesTuple>(nf);
        st->modes.temp = k.take<char>(st->modes.temp_bytes);
        st->modes_recs = k.take<adsb_modes_rec>(nf);
    });
    if (rc != ADSB_OK || !pinned_make(st->modes_pinned, nf) ||
        adsbk::launch_track_modes_clear(st->ctx->aux, st->dev.modes, st->places()) != hipSuccess ||
        hipStreamSynchronize(st->ctx->aux) != hipSuccess) {
        (void)hipGetLastError();
        store_modes_drop(*st);
        return ADSB_E_NOMEM;
    }
    return ADSB_OK;
}

// ---- Comm-B registers per aircraft ------------------------------------------------------------------------------------
// Waits for the device (the clear); a second reserve keeps what the first one made, its cfg too
static int store_commb_reserve(TrackStore *st, const adsb_commb_settle_cfg &cfg)
{
    HIPCHK(hipSetDevice(st->ctx->cfg.device));
    if (st->dev.commb) return ADSB_OK;
    const size_t nf = (size_t)st->max_frames;
    st->commb.temp_bytes = adsbk::track_commb_temp_bytes(nf);
    st->commb.cfg = cfg;
    const int rc = carve_block(st->ctx, st->commb_mem, [&](Carve &k) {
        st->dev.commb = k.take<adsb_aircraft_commb>(st->places());
        st->commb.ref = k.take<adsbk::TrackCommbRefTuple>(nf);
        st->commb.out = k.take<adsb_commb_rec>(nf);
        st->commb.in = k.take<adsbk::TrackCommbTuple>(nf);
        st->commb.scan = k.take<adsbk::TrackCommbTuple>(nf);
        st->commb.temp = k.take<char>(st->commb.temp_bytes);
        st->commb_recs = k.take<adsb_commb_rec>(nf);
    });
    if (rc != ADSB_OK || !pinned_make(st->commb_pinned, nf) ||
        adsbk::launch_track_commb_clear(st->ctx->aux, st->dev.commb, st->places()) != hipSuccess ||
        hipStreamSynchronize(st->ctx->aux) != hipSuccess) {
        (void)hipGetLastError();
        store_commb_drop(*st);
        return ADSB_E_NOMEM;
    }
    return ADSB_OK;
}

// ---- Extended squitter status per aircraft ---------------------------------------------------------------------------
// Waits for the device (the clear); a second reserve keeps what the first one made, its cfg too
static int store_es_reserve(TrackStore *st, double max_age_s)
{
    HIPCHK(hipSetDevice(st->ctx->cfg.device));
    if (st->dev.es) return ADSB_OK;
    const size_t nf = (size_t)st->max_frames;
    st->es.temp_bytes = adsbk::track_es_temp_bytes(nf);
    st->es.max_age_s = max_age_s;
    const int rc = carve_block(st->ctx, st->es_mem, [&](Carve &k) {
        st->dev.es = k.take<adsb_aircraft_es>(st->places());
        st->es.ref = k.take<adsbk::TrackEsRefTuple>(nf);
        st->es.out = k.take<adsb_frame_integrity>(nf);
        st->es.in = k.take<adsbk::TrackEsTuple>(nf);
        st->es.scan = k.take<adsbk::TrackEsTuple>(nf);
        st->es.temp = k.take<char>(st->es.temp_bytes);
        st->es_recs = k.take<adsb_es_rec>(nf);
    });
    if (rc != ADSB_OK || !pinned_make(st->es_pinned, nf) ||
        adsbk::launch_track_es_clear(st->ctx->aux, st->dev.es, st->places()) != hipSuccess ||
        hipStreamSynchronize(st->ctx->aux) != hipSuccess) {
        (void)hipGetLastError();
        store_es_drop(*st);
        return ADSB_E_NOMEM;
    }
    return ADSB_OK;
}

// ---- persistent aircraft table (adsb_track_table_*) ------------------------------------------------------------------
static void track_table_free(adsb_track_table *t)
{
    store_release(*t);
    delete t;
}

extern "C" int adsb_track_table_reset(adsb_track_table *t) { return store_reset(t); }

extern "C" int adsb_track_table_create(adsb_ctx *c, const adsb_track_table_cfg *cfg, adsb_track_table **out)
{
    if (!c || !cfg || !out || cfg->abi_version != ADSB_ABI_VERSION) return ADSB_E_ARG;
    if (cfg->max_frames == 0 || cfg->max_frames > 0xFFFFFFFFull || !(cfg->seconds_per_sample > 0.0) ||
        cfg->max_aircraft > (1u << 24))
        return ADSB_E_ARG;
    *out = nullptr;
    HIPCHK(hipSetDevice(c->cfg.device));
    adsb_track_table *t = new (std::nothrow) adsb_track_table;
    if (!t) return ADSB_E_NOMEM;
    const bool ok = store_alloc(*t, c, TrackKind::kTable, 1, cfg->max_aircraft ? cfg->max_aircraft : 65536u, cfg->max_frames,
                                cfg->seconds_per_sample, adsbk::track_sort_temp_bytes((size_t)cfg->max_frames));
    return store_created(t, ok, track_table_free, out);
}

extern "C" void adsb_track_table_destroy(adsb_track_table *t)
{
    if (t) track_table_free(t);
}

// levels: null for the plain update; fixes: null unless update_mlat (or update_modes with fixes); recs: null unless
// update_modes; commb: null unless update_commb; es: null unless update_es
static int track_table_update(adsb_track_table *t, const adsb_frame *frames, const adsb_frame_level *levels, size_t n,
                              uint64_t sample_base, const adsb_mlat_fix *fixes = nullptr,
                              const adsb_modes_rec *recs = nullptr, const adsb_commb_rec *commb = nullptr,
                              const adsb_es_rec *es = nullptr)
{
    if (n > t->max_frames) return ADSB_E_CAPACITY;
    adsb_ctx *c = t->ctx;
    HIPCHK(hipSetDevice(c->cfg.device));
    if (fixes) store_mlat_list(*t, n);
    if (!store_begin_update(*t, n)) return ADSB_OK;
    const adsb_frame *list = frames;
    const bool frames_host = !in_device_memory(c, frames), levels_host = levels && !in_device_memory(c, levels);
    const bool fixes_host = fixes && !in_device_memory(c, fixes), recs_host = recs && !in_device_memory(c, recs);
    const bool commb_host = commb && !in_device_memory(c, commb), es_host = es && !in_device_memory(c, es);
    if (es) { // the list fetch_frame_es speaks of
        t->es_n = (uint32_t)n;
        t->es_updated = true;
    }
    if (commb) { // the list fetch_frame_commb speaks of
        t->commb_n = (uint32_t)n;
        t->commb_updated = true;
    }
    if (frames_host || levels_host || fixes_host || recs_host || commb_host || es_host) {
        HIPCHK(hipEventSynchronize(t->copied)); // the previous update's copies out of the staging have finished
        int rc = frames_host ? store_stage_frames(*t, frames, n) : ADSB_OK;
        if (rc == ADSB_OK && levels_host) rc = store_stage_levels(*t, levels, n);
        if (rc == ADSB_OK && fixes_host) rc = store_stage_mlat(*t, fixes, n);
        if (rc == ADSB_OK && recs_host) rc = store_stage_modes(*t, recs, n);
        if (rc == ADSB_OK && commb_host) rc = store_stage_commb(*t, commb, n);
        if (rc == ADSB_OK && es_host) rc = store_stage_es(*t, es, n);
        if (rc != ADSB_OK) return rc;
        HIPCHK(hipEventRecord(t->copied, c->aux));
        if (frames_host) list = t->frames;
        if (levels_host) levels = t->lvl_frames;
        if (fixes_host) fixes = t->mlat_fixes;
        if (recs_host) recs = t->modes_recs;
        if (commb_host) commb = t->commb_recs;
        if (es_host) es = t->es_recs;
    }
    return store_run(*t, list, n, sample_base, t->dev, levels, fixes, recs, commb, es);
}

extern "C" int adsb_track_table_update(adsb_track_table *t, const adsb_frame *frames, size_t n, uint64_t sample_base)
{
    if (!t || (!frames && n)) return ADSB_E_ARG;
    return track_table_update(t, frames, nullptr, n, sample_base);
}

extern "C" int adsb_track_table_levels_reserve(adsb_track_table *t) { return store_levels_reserve(t); }

extern "C" int adsb_track_table_update_levels(adsb_track_table *t, const adsb_frame *frames,
                                              const adsb_frame_level *levels, size_t n, uint64_t sample_base)
{
    if (!t || (!frames && n) || (!levels && n)) return ADSB_E_ARG;
    if (!t->dev.lvl) return ADSB_E_STATE;
    return track_table_update(t, frames, n ? levels : nullptr, n, sample_base);
}

extern "C" int adsb_track_table_fetch_levels(adsb_track_table *t, adsb_aircraft_level *out, size_t max, size_t *n)
{
    return store_fetch_side(t, levels_of, out, max, n);
}

extern "C" int adsb_track_table_levels_device(adsb_track_table *t, const adsb_aircraft_level **dev)
{
    return store_device(t, levels_of, dev);
}

extern "C" int adsb_track_table_fixes_reserve(adsb_track_table *t, const adsb_site *site)
{
    if (!t || !site || !adsbk::fix_site_ok(*site)) return ADSB_E_ARG; // before the handle is read
    return store_fixes_reserve(t, site);
}

extern "C" int adsb_track_table_fetch_fixes(adsb_track_table *t, adsb_fix *out, size_t max, size_t *n)
{
    return store_fetch_side(t, fixes_of, out, max, n);
}

extern "C" int adsb_track_table_fixes_device(adsb_track_table *t, const adsb_fix **dev)
{
    return store_device(t, fixes_of, dev);
}

extern "C" int adsb_track_table_fetch_frame_fixes(adsb_track_table *t, adsb_frame_fix *out, size_t max, size_t *n)
{
    return store_fetch_frames(t, frame_fixes_of, out, max, n, Report::kCopied);
}

extern "C" int adsb_track_table_mlat_reserve(adsb_track_table *t, double max_disagreement_m)
{
    if (!t || !std::isfinite(max_disagreement_m) || !(max_disagreement_m > 0.0)) return ADSB_E_ARG; // before the handle is read
    return store_mlat_reserve(t, max_disagreement_m);
}

extern "C" int adsb_track_table_update_mlat(adsb_track_table *t, const adsb_frame *frames, const adsb_mlat_fix *fixes,
                                            const adsb_frame_level *levels, size_t n, uint64_t sample_base)
{
    if (!t || (!frames && n) || (!fixes && n)) return ADSB_E_ARG;
    if (!t->dev.mlat || (levels && !t->dev.lvl)) return ADSB_E_STATE;
    if (n > t->max_frames) return ADSB_E_CAPACITY;
    if (n == 0) store_mlat_list(*t, 0); // nothing to launch: the last update_mlat's list is empty
    return track_table_update(t, frames, n ? levels : nullptr, n, sample_base, n ? fixes : nullptr);
}

extern "C" int adsb_track_table_fetch_mlat(adsb_track_table *t, adsb_aircraft_mlat *out, size_t max, size_t *n)
{
    return store_fetch_side(t, mlat_of, out, max, n);
}

extern "C" int adsb_track_table_mlat_device(adsb_track_table *t, const adsb_aircraft_mlat **dev)
{
    return store_device(t, mlat_of, dev);
}

extern "C" int adsb_track_table_filter_reserve(adsb_track_table *t, const adsb_track_filter_cfg *cfg)
{
    adsb_track_filter_cfg use;
    if (!t || !adsbk::filter_cfg_resolve(cfg, use)) return ADSB_E_ARG; // before the handle is read
    return store_filter_reserve(t, use);
}

extern "C" int adsb_track_table_fetch_filter(adsb_track_table *t, adsb_aircraft_filter *out, size_t max, size_t *n)
{
    return store_fetch_side(t, filter_of, out, max, n);
}

extern "C" int adsb_track_table_filter_device(adsb_track_table *t, const adsb_aircraft_filter **dev)
{
    return store_device(t, filter_of, dev);
}

// Waits.  The first min(list, max) records of a per-frame array of the filter, over the last update given fixes
template <class T>
static int table_fetch_filter_frames(adsb_track_table *t, const T *src, T *out, size_t max, size_t *n)
{
    if (!t || (!out && max)) return ADSB_E_ARG;
    if (!t->dev.filter || !t->filter_updated) return ADSB_E_STATE;
    HIPCHK(hipSetDevice(t->ctx->cfg.device));
    const size_t take = std::min<size_t>(t->mlat_n, max);
    if (take) HIPCHK(hipMemcpyAsync(out, src, sizeof(T) * take, hipMemcpyDeviceToHost, t->ctx->aux));
    HIPCHK(hipStreamSynchronize(t->ctx->aux));
    if (n) *n = take;
    return ADSB_OK;
}

extern "C" int adsb_track_table_fetch_frame_filter(adsb_track_table *t, adsb_frame_filter *out, size_t max, size_t *n)
{
    return table_fetch_filter_frames(t, t ? t->filter.out : nullptr, out, max, n);
}

extern "C" int adsb_debug_track_filter_operands(adsb_track_table *t, adsb_filter_operand *out, size_t max, size_t *n)
{
    return table_fetch_filter_frames(t, t ? t->filter.op : nullptr, out, max, n);
}

extern "C" int adsb_track_table_modes_reserve(adsb_track_table *t)
{
    if (!t) return ADSB_E_ARG;
    return store_modes_reserve(t);
}

extern "C" int adsb_track_table_update_modes(adsb_track_table *t, const adsb_frame *frames, const adsb_modes_rec *recs,
                                             const adsb_mlat_fix *fixes, const adsb_frame_level *levels, size_t n,
                                             uint64_t sample_base)
{
    if (!t || (!frames && n) || (!recs && n)) return ADSB_E_ARG;
    if (!t->dev.modes || (fixes && !t->dev.mlat) || (levels && !t->dev.lvl)) return ADSB_E_STATE;
    if (n > t->max_frames) return ADSB_E_CAPACITY;
    if (n == 0 && fixes) store_mlat_list(*t, 0); // nothing to launch: the last update with fixes has an empty list
    return track_table_update(t, frames, n ? levels : nullptr, n, sample_base, n ? fixes : nullptr, n ? recs : nullptr);
}

extern "C" int adsb_track_table_fetch_modes(adsb_track_table *t, adsb_aircraft_modes *out, size_t max, size_t *n)
{
    return store_fetch_side(t, modes_of, out, max, n);
}

extern "C" int adsb_track_table_modes_device(adsb_track_table *t, const adsb_aircraft_modes **dev)
{
    return store_device(t, modes_of, dev);
}

extern "C" int adsb_track_table_commb_reserve(adsb_track_table *t, const adsb_commb_settle_cfg *cfg)
{
    const adsb_commb_settle_cfg use = cfg ? *cfg : adsb_commb_settle_cfg{10.0, 40u, 1000u};
    if (!t || !(use.max_age_s >= 0.0)) return ADSB_E_ARG; // before the handle is read
    return store_commb_reserve(t, use);
}

extern "C" int adsb_track_table_update_commb(adsb_track_table *t, const adsb_frame *frames, const adsb_modes_rec *recs,
                                             const adsb_commb_rec *commb, const adsb_mlat_fix *fixes,
                                             const adsb_frame_level *levels, size_t n, uint64_t sample_base)
{
    if (!t || (!frames && n) || (!recs && n) || (!commb && n)) return ADSB_E_ARG;
    if (!t->dev.modes || !t->dev.commb || (fixes && !t->dev.mlat) || (levels && !t->dev.lvl)) return ADSB_E_STATE;
    if (n > t->max_frames) return ADSB_E_CAPACITY;
    if (n == 0) { // nothing to launch: the last update_commb's list is empty
        t->commb_n = 0;
        t->commb_updated = true;
        if (fixes) store_mlat_list(*t, 0);
    }
    return track_table_update(t, frames, n ? levels : nullptr, n, sample_base, n ? fixes : nullptr, n ? recs : nullptr,
                              n ? commb : nullptr);
}

extern "C" int adsb_track_table_fetch_commb(adsb_track_table *t, adsb_aircraft_commb *out, size_t max, size_t *n)
{
    return store_fetch_side(t, commb_of, out, max, n);
}

extern "C" int adsb_track_table_commb_device(adsb_track_table *t, const adsb_aircraft_commb **dev)
{
    return store_device(t, commb_of, dev);
}

// Waits.  As fetch_frame_mlat, over the last update_commb's list
extern "C" int adsb_track_table_fetch_frame_commb(adsb_track_table *t, adsb_commb_rec *out, size_t max, size_t *n)
{
    if (!t || (!out && max)) return ADSB_E_ARG;
    if (!t->dev.commb || !t->commb_updated) return ADSB_E_STATE;
    HIPCHK(hipSetDevice(t->ctx->cfg.device));
    const size_t take = std::min<size_t>(t->commb_n, max);
    if (take) HIPCHK(hipMemcpyAsync(out, t->commb.out, sizeof(adsb_commb_rec) * take, hipMemcpyDeviceToHost, t->ctx->aux));
    HIPCHK(hipStreamSynchronize(t->ctx->aux));
    if (n) *n = take;
    return ADSB_OK;
}

extern "C" int adsb_track_table_es_reserve(adsb_track_table *t, const adsb_es_track_cfg *cfg)
{
    const double max_age_s = cfg ? cfg->max_age_s : 60.0;
    if (!t || !(max_age_s >= 0.0)) return ADSB_E_ARG; // before the handle is read
    return store_es_reserve(t, max_age_s);
}

// recs NULL: the plain update (with levels: update_levels, with fixes: update_mlat); recs: update_modes; recs and commb:
// update_commb; each with the es step
extern "C" int adsb_track_table_update_es(adsb_track_table *t, const adsb_frame *frames, const adsb_es_rec *es,
                                          const adsb_modes_rec *recs, const adsb_commb_rec *commb,
                                          const adsb_mlat_fix *fixes, const adsb_frame_level *levels, size_t n,
                                          uint64_t sample_base)
{
    if (!t || (!frames && n) || (!es && n) || (commb && !recs)) return ADSB_E_ARG;
    if (!t->dev.es || (recs && !t->dev.modes) || (commb && !t->dev.commb) || (fixes && !t->dev.mlat) ||
        (levels && !t->dev.lvl))
        return ADSB_E_STATE;
    if (n > t->max_frames) return ADSB_E_CAPACITY;
    if (n == 0) { // nothing to launch: the last update's lists are empty
        t->es_n = 0;
        t->es_updated = true;
        if (commb) {
            t->commb_n = 0;
            t->commb_updated = true;
        }
        if (fixes) store_mlat_list(*t, 0);
    }
    return track_table_update(t, frames, n ? levels : nullptr, n, sample_base, n ? fixes : nullptr, n ? recs : nullptr,
                              n ? commb : nullptr, n ? es : nullptr);
}

extern "C" int adsb_track_table_fetch_es(adsb_track_table *t, adsb_aircraft_es *out, size_t max, size_t *n)
{
    return store_fetch_side(t, es_of, out, max, n);
}

extern "C" int adsb_track_table_es_device(adsb_track_table *t, const adsb_aircraft_es **dev)
{
    return store_device(t, es_of, dev);
}

// Waits.  As fetch_frame_commb, over the last update_es's list
extern "C" int adsb_track_table_fetch_frame_es(adsb_track_table *t, adsb_frame_integrity *out, size_t max, size_t *n)
{
    if (!t || (!out && max)) return ADSB_E_ARG;
    if (!t->dev.es || !t->es_updated) return ADSB_E_STATE;
    HIPCHK(hipSetDevice(t->ctx->cfg.device));
    const size_t take = std::min<size_t>(t->es_n, max);
    if (take) HIPCHK(hipMemcpyAsync(out, t->es.out, sizeof(adsb_frame_integrity) * take, hipMemcpyDeviceToHost, t->ctx->aux));
    HIPCHK(hipStreamSynchronize(t->ctx->aux));
    if (n) *n = take;
    return ADSB_OK;
}

// Waits.  As store_fetch_frames, over the last update_mlat's list (a plain update in between leaves it alone)
extern "C" int adsb_track_table_fetch_frame_mlat(adsb_track_table *t, adsb_frame_mlat *out, size_t max, size_t *n)
{
    if (!t || (!out && max)) return ADSB_E_ARG;
    if (!t->dev.mlat || !t->mlat_updated) return ADSB_E_STATE;
    HIPCHK(hipSetDevice(t->ctx->cfg.device));
    const size_t take = std::min<size_t>(t->mlat_n, max);
    if (take) HIPCHK(hipMemcpyAsync(out, t->mlat.out, sizeof(adsb_frame_mlat) * take, hipMemcpyDeviceToHost, t->ctx->aux));
    HIPCHK(hipStreamSynchronize(t->ctx->aux));
    if (n) *n = take;
    return ADSB_OK;
}

extern "C" int adsb_track_table_summaries_reserve(adsb_track_table *t) { return store_summaries_reserve(t); }

extern "C" int adsb_track_table_fetch_summaries(adsb_track_table *t, adsb_aircraft_record *out, size_t max, size_t *n)
{
    return store_fetch_frames(t, summaries_of, out, max, n, Report::kListLength);
}

extern "C" int adsb_track_table_summaries_device(adsb_track_table *t, const adsb_aircraft_record **dev)
{
    return store_device(t, summaries_of, dev);
}

extern "C" int adsb_track_table_fetch_changed(adsb_track_table *t, adsb_aircraft_record *rec, double *last_heard,
                                              adsb_velocity *velocity, size_t max, size_t *n)
{
    return store_fetch_changed(t, rec, last_heard, velocity, max, n, nullptr);
}

extern "C" int adsb_track_table_fetch_points(adsb_track_table *t, adsb_track_point *points, size_t max_points,
                                             size_t *n_points)
{
    return store_fetch_frames(t, points_of, points, max_points, n_points, Report::kCopied);
}

extern "C" int adsb_track_table_fetch(adsb_track_table *t, adsb_aircraft_record *aircraft, size_t max_aircraft,
                                      size_t *n_aircraft, uint32_t *flags)
{
    return store_fetch(t, aircraft, max_aircraft, n_aircraft, nullptr, flags, record_of);
}

extern "C" int adsb_track_table_expire(adsb_track_table *t, double before)
{
    if (!t || std::isnan(before)) return ADSB_E_ARG; // before the handle is read
    return store_expire(t, &before);
}

extern "C" int adsb_track_table_fetch_last_heard(adsb_track_table *t, double *last_heard, size_t max, size_t *n)
{
    return store_fetch(t, last_heard, max, n, nullptr, nullptr, last_heard_of);
}

extern "C" int adsb_track_table_fetch_velocity(adsb_track_table *t, adsb_velocity *velocity, size_t max, size_t *n)
{
    return store_fetch(t, velocity, max, n, nullptr, nullptr, velocity_of);
}

// ---- a bank of persistent tables, one per receiver (adsb_track_bank_*) ----------------------------------------------
// The fuse reserve gone.  The caller has waited for the fuse that may still use it.
static void track_bank_fuse_drop(adsb_track_bank *b)
{
    drop(b->fuse_mem);
    drop(b->fuse_lvl_out);
    b->fuse = {};
}

static void track_bank_free(adsb_track_bank *b)
{
    store_release(*b);
    track_bank_fuse_drop(b);
    delete b;
}

extern "C" int adsb_track_bank_reset(adsb_track_bank *b) { return store_reset(b); }

extern "C" int adsb_track_bank_create(adsb_ctx *c, const adsb_track_bank_cfg *cfg, adsb_track_bank **out)
{
    if (!c || !cfg || !out || cfg->abi_version != ADSB_ABI_VERSION || cfg->reserved != 0) return ADSB_E_ARG;
    if (cfg->n_receivers == 0 || cfg->n_receivers > adsbk::kMaxReceivers || cfg->max_frames == 0 || cfg->max_frames > 0xFFFFFFFFull ||
        !(cfg->seconds_per_sample > 0.0) || cfg->max_aircraft > (1u << 24))
        return ADSB_E_ARG;
    *out = nullptr;
    const uint32_t nr = cfg->n_receivers, max_ac = cfg->max_aircraft ? cfg->max_aircraft : 65536u;
    const uint64_t n_rec = (uint64_t)nr * max_ac;
    if (n_rec >= 0xFFFFFFFFull) return ADSB_E_NOMEM; // slot + 1 must fit 32 bits: 2^32 records would need > 350 GiB
    HIPCHK(hipSetDevice(c->cfg.device));
    adsb_track_bank *b = new (std::nothrow) adsb_track_bank;
    if (!b) return ADSB_E_NOMEM;
    uint64_t cap = 1;
    while (cap < 2 * n_rec) cap <<= 1;
    b->dev.hash_mask = cap - 1;
    uint32_t bits = 0;
    while ((1u << bits) < nr) ++bits;
    b->dev.key_bits = 24 + bits;
    const bool ok = store_alloc(*b, c, TrackKind::kBank, nr, max_ac, cfg->max_frames, cfg->seconds_per_sample,
                                adsbk::track_bank_temp_bytes((size_t)cfg->max_frames));
    return store_created(b, ok, track_bank_free, out);
}

extern "C" void adsb_track_bank_destroy(adsb_track_bank *b)
{
    if (b) track_bank_free(b);
}

// Enqueues the bank's kernels over n frames at `list` (device) with the receiver split src_prefix[0..n_src]; meta's
// sample_base part has been filled by the caller (and the staging copy enqueued).
static int track_bank_run(adsb_track_bank *b, const adsb_frame *list, size_t n, const uint64_t *src_prefix,
                          uint32_t n_src, const adsb_frame_level *levels = nullptr)
{
    adsbk::TrackStoreDev dev = b->dev;
    dev.src_prefix = src_prefix;
    dev.n_src = n_src;
    return store_run(*b, list, n, 0, dev, levels);
}

// Stages sample_base (and, for a host split, the counts' prefix) through meta_pinned; frames_host / levels_host: also
// the frames / the level records.
static int track_bank_stage(adsb_track_bank *b, const uint64_t *counts, const uint64_t *sample_base,
                            const adsb_frame *frames_host, size_t n, const adsb_frame_level *levels_host = nullptr)
{
    adsb_ctx *c = b->ctx;
    const uint32_t nr = b->n_receivers;
    HIPCHK(hipEventSynchronize(b->copied)); // the previous update's copies out of the staging have finished
    uint64_t *m = b->meta_pinned;
    m[0] = 0;
    for (uint32_t r = 0; r < nr; ++r) {
        m[r + 1] = m[r] + (counts ? counts[r] : 0);
        m[nr + 1 + r] = sample_base ? sample_base[r] : 0;
    }
    HIPCHK(hipMemcpyAsync(b->meta, m, sizeof(uint64_t) * (2 * nr + 1), hipMemcpyHostToDevice, c->aux));
    if (frames_host) {
        int rc = store_stage_frames(*b, frames_host, n);
        if (rc != ADSB_OK) return rc;
    }
    if (levels_host) {
        int rc = store_stage_levels(*b, levels_host, n);
        if (rc != ADSB_OK) return rc;
    }
    HIPCHK(hipEventRecord(b->copied, c->aux));
    return ADSB_OK;
}

// levels: null for the plain update
static int track_bank_update(adsb_track_bank *b, const adsb_frame *frames, const adsb_frame_level *levels, size_t n,
                             const uint64_t *counts, const uint64_t *sample_base)
{
    if (counts) {
        uint64_t sum = 0;
        for (uint32_t r = 0; r < b->n_receivers; ++r) {
            if (counts[r] > n - sum) return ADSB_E_ARG;
            sum += counts[r];
        }
        if (sum != n) return ADSB_E_ARG;
    }
    if (n > b->max_frames) return ADSB_E_CAPACITY;
    adsb_ctx *c = b->ctx;
    HIPCHK(hipSetDevice(c->cfg.device));
    if (!store_begin_update(*b, n)) return ADSB_OK;
    const bool on_device = in_device_memory(c, frames), levels_host = levels && !in_device_memory(c, levels);
    int rc = track_bank_stage(b, counts, sample_base, on_device ? nullptr : frames, n, levels_host ? levels : nullptr);
    if (rc != ADSB_OK) return rc;
    return track_bank_run(b, on_device ? frames : b->frames, n, b->meta, b->n_receivers,
                          levels_host ? b->lvl_frames : levels);
}

extern "C" int adsb_track_bank_update(adsb_track_bank *b, const adsb_frame *frames, size_t n, const uint64_t *counts,
                                      const uint64_t *sample_base)
{
    if (!b || (!frames && n) || (!counts && n)) return ADSB_E_ARG;
    return track_bank_update(b, frames, nullptr, n, counts, sample_base);
}

extern "C" int adsb_track_bank_levels_reserve(adsb_track_bank *b)
{
    int rc = store_levels_reserve(b);
    if (rc != ADSB_OK || !b->fuse.max || b->fuse_lvl_out.p) return rc;
    // the fuse reserve came first: the fused level records are this reserve's to make
    if (replace(b->ctx, b->fuse_lvl_out, b->fuse.max) != ADSB_OK) {
        store_levels_drop(*b);
        return ADSB_E_NOMEM;
    }
    return ADSB_OK;
}

extern "C" int adsb_track_bank_update_levels(adsb_track_bank *b, const adsb_frame *frames,
                                             const adsb_frame_level *levels, size_t n, const uint64_t *counts,
                                             const uint64_t *sample_base)
{
    if (!b || (!frames && n) || (!levels && n) || (!counts && n)) return ADSB_E_ARG;
    if (!b->dev.lvl) return ADSB_E_STATE;
    return track_bank_update(b, frames, n ? levels : nullptr, n, counts, sample_base);
}

extern "C" int adsb_track_bank_fetch_levels(adsb_track_bank *b, adsb_aircraft_level *out, size_t max, size_t *n)
{
    return store_fetch_side(b, levels_of, out, max, n);
}

extern "C" int adsb_track_bank_levels_device(adsb_track_bank *b, const adsb_aircraft_level **dev)
{
    return store_device(b, levels_of, dev);
}

// with_levels: also the ctx's levels of the same launch (adsb_track_bank_update_launch_levels)
static int track_bank_update_launch(adsb_track_bank *b, const uint64_t *sample_base, bool with_levels)
{
    adsb_ctx *c = b->ctx;
    if (!c->launched) return ADSB_E_STATE;
    if (c->launch().channels > b->n_receivers) return ADSB_E_ARG;
    int rc = sync_header(c); // the list's length, as adsb_fetch_counts (and the rebuild after a slot-pool overflow)
    if (rc != ADSB_OK) return rc;
    const uint64_t n = std::min<uint64_t>(c->hdr_host->n_out, c->launch().cap);
    if (n > b->max_frames) return ADSB_E_CAPACITY;
    HIPCHK(hipSetDevice(c->cfg.device));
    // not enqueued yet for this launch, or of the list with holes that sync_header has just rebuilt: (again) now, on
    // the stream the tracker's kernels follow on; before the store's bookkeeping, which an error here leaves as it was
    if (with_levels && n && !(c->levels && c->levels_current) && (rc = adsb_levels_device_async(c)) != ADSB_OK) return rc;
    if (!store_begin_update(*b, (size_t)n)) return ADSB_OK;
    if ((rc = track_bank_stage(b, nullptr, sample_base, nullptr, 0)) != ADSB_OK) return rc;
    adsb_ctx::ResultSet &r = c->rs[c->last];
    // the channel split as adsb_fetch's per_channel_counts reads it: chan_prefix clipped to the list
    if ((rc = track_bank_run(b, c->launch().out, (size_t)n, r.chan_prefix, c->launch().channels,
                             with_levels ? c->levels : nullptr)) != ADSB_OK)
        return rc;
    if (c->own_aux) { // the launch that reuses this result set waits for these kernels too
        HIPCHK(hipEventRecord(r.g_done, c->aux));
        r.g_pending = true;
    }
    return ADSB_OK;
}

extern "C" int adsb_track_bank_update_launch(adsb_track_bank *b, const uint64_t *sample_base)
{
    if (!b) return ADSB_E_ARG;
    return track_bank_update_launch(b, sample_base, false);
}

extern "C" int adsb_track_bank_update_launch_levels(adsb_track_bank *b, const uint64_t *sample_base)
{
    if (!b) return ADSB_E_ARG;
    if (!b->dev.lvl) return ADSB_E_STATE;
    return track_bank_update_launch(b, sample_base, true);
}

extern "C" int adsb_track_bank_fetch_points(adsb_track_bank *b, adsb_track_point *points, size_t max_points,
                                            size_t *n_points)
{
    return store_fetch_frames(b, points_of, points, max_points, n_points, Report::kCopied);
}

extern "C" int adsb_track_bank_fetch(adsb_track_bank *b, adsb_aircraft_record *aircraft, size_t max_aircraft,
                                     size_t *n_aircraft, uint64_t *per_receiver_counts, uint32_t *flags)
{
    return store_fetch(b, aircraft, max_aircraft, n_aircraft, per_receiver_counts, flags, record_of);
}

extern "C" int adsb_track_bank_expire(adsb_track_bank *b, const double *before) { return store_expire(b, before); }

extern "C" int adsb_track_bank_fixes_reserve(adsb_track_bank *b, const adsb_site *sites)
{
    if (!b || !sites) return ADSB_E_ARG;
    for (uint32_t r = 0; r < b->n_receivers; ++r)
        if (!adsbk::fix_site_ok(sites[r])) return ADSB_E_ARG;
    return store_fixes_reserve(b, sites);
}

extern "C" int adsb_track_bank_fetch_fixes(adsb_track_bank *b, adsb_fix *out, size_t max, size_t *n)
{
    return store_fetch_side(b, fixes_of, out, max, n);
}

extern "C" int adsb_track_bank_fixes_device(adsb_track_bank *b, const adsb_fix **dev)
{
    return store_device(b, fixes_of, dev);
}

extern "C" int adsb_track_bank_fetch_frame_fixes(adsb_track_bank *b, adsb_frame_fix *out, size_t max, size_t *n)
{
    return store_fetch_frames(b, frame_fixes_of, out, max, n, Report::kCopied);
}

extern "C" int adsb_track_bank_summaries_reserve(adsb_track_bank *b) { return store_summaries_reserve(b); }

extern "C" int adsb_track_bank_fetch_summaries(adsb_track_bank *b, adsb_aircraft_record *out, size_t max, size_t *n)
{
    return store_fetch_frames(b, summaries_of, out, max, n, Report::kListLength);
}

extern "C" int adsb_track_bank_summaries_device(adsb_track_bank *b, const adsb_aircraft_record **dev)
{
    return store_device(b, summaries_of, dev);
}

extern "C" int adsb_track_bank_fetch_changed(adsb_track_bank *b, adsb_aircraft_record *rec, double *last_heard,
                                             adsb_velocity *velocity, size_t max, size_t *n,
                                             uint64_t *per_receiver_counts)
{
    return store_fetch_changed(b, rec, last_heard, velocity, max, n, per_receiver_counts);
}

extern "C" int adsb_track_bank_fetch_last_heard(adsb_track_bank *b, double *last_heard, size_t max, size_t *n)
{
    return store_fetch(b, last_heard, max, n, nullptr, nullptr, last_heard_of);
}

extern "C" int adsb_track_bank_fetch_velocity(adsb_track_bank *b, adsb_velocity *velocity, size_t max, size_t *n)
{
    return store_fetch(b, velocity, max, n, nullptr, nullptr, velocity_of);
}

// ---- the fused view of a bank: one record per ICAO over all receivers (adsb_track.hip, launch_track_fuse) ----
extern "C" int adsb_track_bank_fuse_reserve(adsb_track_bank *b, size_t max_fused)
{
    if (!b) return ADSB_E_ARG;
    adsb_ctx *c = b->ctx;
    HIPCHK(hipSetDevice(c->cfg.device));
    HIPCHK(hipStreamSynchronize(c->aux)); // a fuse may still read what is freed here
    track_bank_fuse_drop(b);
    adsb_track_bank::Fuse &f = b->fuse;
    const uint32_t nr = b->n_receivers;
    const size_t places = b->places();
    const size_t cap = max_fused == 0 || max_fused > places ? places : max_fused; // more than `places` cannot occur
    const size_t key_bytes = nr > adsbk::kFuseWideReceivers ? sizeof(uint64_t) : sizeof(uint32_t);
    f.temp_bytes = adsbk::track_fuse_temp_bytes(places, nr);
    f.lanes = nr == 1 ? 1u : 4u; // measured: DESIGN 4.4f (16 and 64 lanes lost on runs of 64 and of 1 alike)
    if (const char *fl = getenv("ADSB_FUSE_LANES")) { // measurement knob: lanes per ICAO in the reduction
        const int v = atoi(fl);
        if (v == 1 || v == 4) f.lanes = (uint32_t)v;
    }
    int rc = carve_block(c, b->fuse_mem, [&](Carve &k) {
        f.keys = k.take<char>(2 * key_bytes * places);
        f.vals = k.take<uint32_t>(2 * places);
        f.start = k.take<uint32_t>(cap);
        f.out = k.take<adsb_fused_aircraft>(cap);
        f.counts = k.take<uint64_t>(3);
        f.temp = k.take<char>(f.temp_bytes);
    });
    if (rc == ADSB_OK && b->dev.lvl) rc = replace(c, b->fuse_lvl_out, cap); // the levels reserve came first
    if (rc != ADSB_OK) {
        track_bank_fuse_drop(b);
        return ADSB_E_NOMEM;
    }
    f.max = cap;
    return ADSB_OK;
}

extern "C" int adsb_track_bank_fuse(adsb_track_bank *b, double since)
{
    if (!b || std::isnan(since)) return ADSB_E_ARG;
    if (!b->fuse.max) return ADSB_E_STATE;
    HIPCHK(hipSetDevice(b->ctx->cfg.device));
    const size_t places = b->places();
    const size_t key_bytes = b->n_receivers > adsbk::kFuseWideReceivers ? sizeof(uint64_t) : sizeof(uint32_t);
    adsbk::FuseArgs a{};
    a.bank = &b->dev;
    a.since = since;                 // by value in the kernel's arguments, as expire's cuts: no staging, no wait
    a.keys = b->fuse.keys;
    a.skeys = (char *)b->fuse.keys + key_bytes * places;
    a.vals = b->fuse.vals;
    a.svals = b->fuse.vals + places;
    a.seg_start = b->fuse.start;
    a.out = b->fuse.out;
    a.lvl_out = b->dev.lvl ? b->fuse_lvl_out.p : nullptr; // both reserves: the fused levels too
    a.counts = b->fuse.counts;
    a.max_fused = b->fuse.max;
    a.temp = b->fuse.temp;
    a.temp_bytes = b->fuse.temp_bytes;
    a.lanes = b->fuse.lanes;
    HIPCHK(adsbk::launch_track_fuse(b->ctx->aux, a)); // after the bank's last update / expire / reset (same stream)
    b->fuse.fused = true;
    b->fuse.fused_levels = a.lvl_out != nullptr;
    return ADSB_OK;
}

extern "C" int adsb_track_bank_fetch_fused_levels(adsb_track_bank *b, adsb_fused_level *out, size_t max, size_t *n)
{
    if (!b || (!out && max)) return ADSB_E_ARG;
    if (!b->fuse.fused || !b->fuse.fused_levels) return ADSB_E_STATE;
    adsb_ctx *c = b->ctx;
    HIPCHK(hipSetDevice(c->cfg.device));
    uint64_t written = 0;
    HIPCHK(hipMemcpyAsync(&written, b->fuse.counts, sizeof(written), hipMemcpyDeviceToHost, c->aux));
    HIPCHK(hipStreamSynchronize(c->aux));
    written = std::min<uint64_t>(written, b->fuse.max);
    const size_t take = std::min<size_t>((size_t)written, max);
    if (take) {
        HIPCHK(hipMemcpyAsync(out, b->fuse_lvl_out.p, sizeof(adsb_fused_level) * take, hipMemcpyDeviceToHost, c->aux));
        HIPCHK(hipStreamSynchronize(c->aux));
    }
    if (n) *n = (size_t)written;
    return ADSB_OK;
}

extern "C" int adsb_track_bank_fetch_fused(adsb_track_bank *b, adsb_fused_aircraft *out, size_t max, size_t *n,
                                           size_t *n_total, uint32_t *flags)
{
    if (!b || (!out && max)) return ADSB_E_ARG;
    if (!b->fuse.fused) return ADSB_E_STATE;
    adsb_ctx *c = b->ctx;
    HIPCHK(hipSetDevice(c->cfg.device));
    uint64_t w[3];
    HIPCHK(hipMemcpyAsync(w, b->fuse.counts, sizeof(w), hipMemcpyDeviceToHost, c->aux));
    HIPCHK(hipStreamSynchronize(c->aux));
    const size_t take = std::min<size_t>(std::min<uint64_t>(w[0], b->fuse.max), max);
    if (take) {
        HIPCHK(hipMemcpyAsync(out, b->fuse.out, sizeof(adsb_fused_aircraft) * take, hipMemcpyDeviceToHost, c->aux));
        HIPCHK(hipStreamSynchronize(c->aux));
    }
    if (n) *n = take;
    if (n_total) *n_total = (size_t)w[1];
    if (flags) *flags = (uint32_t)w[2];
    return ADSB_OK;
}

extern "C" int adsb_track_bank_fused_device(adsb_track_bank *b, const adsb_fused_aircraft **fused_dev,
                                            const uint64_t **counts_dev)
{
    if (!b) return ADSB_E_ARG;
    if (!b->fuse.fused) return ADSB_E_STATE;
    if (fused_dev) *fused_dev = b->fuse.out;
    if (counts_dev) *counts_dev = b->fuse.counts;
    return ADSB_OK;
}
