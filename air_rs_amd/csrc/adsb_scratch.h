// adsb_scratch.h -- the one rule the C boundary keeps its device scratch by: is a caller's pointer device memory, grow a
// buffer behind the kernels that may still use it, carve one allocation into aligned arrays, and read a caller's list from
// where it lies or through a device copy.  Header-only; internal.
#pragma once
#include <algorithm>

#include "adsb_ctx.h"

static inline bool in_device_memory(const adsb_ctx *c, const void *p)
{
    hipPointerAttribute_t at{};
    const bool yes = hipPointerGetAttributes(&at, p) == hipSuccess && at.type == hipMemoryTypeDevice &&
                     at.device == c->cfg.device;
    (void)hipGetLastError(); // a plain host pointer is an error to the query: do not leave it to the launches after it
    return yes;
}

// b is empty afterwards.  The caller has waited for whatever may still use what it held.
template <class T>
static inline void drop(DevBuf<T> &b)
{
    (void)hipFree(b.p);
    b = DevBuf<T>{};
}

// b holds exactly n records afterwards.  An earlier call's kernels may still use what it held: the host waits for c->aux
// before freeing it, and only then.  ADSB_E_NOMEM leaves b empty.
template <class T>
static inline int replace(adsb_ctx *c, DevBuf<T> &b, size_t n)
{
    if (b.p) HIPCHK(hipStreamSynchronize(c->aux));
    drop(b);
    if (hipMalloc((void **)&b.p, sizeof(T) * n) != hipSuccess) {
        (void)hipGetLastError();
        b = DevBuf<T>{};
        return ADSB_E_NOMEM;
    }
    b.n = n;
    return ADSB_OK;
}

// b holds at least `need` records afterwards (at least one): kept if it is large enough, never shrunk.
template <class T>
static inline int grow(adsb_ctx *c, DevBuf<T> &b, size_t need)
{
    need = std::max<size_t>(need, 1);
    return b.p && b.n >= need ? ADSB_OK : replace(c, b, need);
}

// One allocation carved into arrays that each start 256-byte aligned.  carve_block lays a feature's arrays out twice by
// the same text: from base 0 for the total, then from the block that total was allocated for.
struct Carve {
    uintptr_t base = 0;
    size_t total = 0;
    template <class T>
    T *take(size_t n)
    {
        T *p = reinterpret_cast<T *>(base + total);
        total += (sizeof(T) * n + 255) & ~(size_t)255;
        return p;
    }
};

// mem becomes one block that `layout(Carve &)` has pointed the owner's arrays into.  After ADSB_E_NOMEM mem is empty and
// those pointers mean nothing.
template <class F>
static inline int carve_block(adsb_ctx *c, DevBuf<char> &mem, F layout)
{
    Carve measure;
    layout(measure);
    const int rc = replace(c, mem, measure.total);
    if (rc != ADSB_OK) return rc;
    Carve place{(uintptr_t)mem.p};
    layout(place);
    return ADSB_OK;
}

// *use = where the kernels read the caller's list of n records: a device list where it lies, a host list in b, grown to
// hold it and filled on c->aux (the caller waits for c->aux before it returns the host list).
template <class T>
static inline int stage_list(adsb_ctx *c, const T *src, size_t n, DevBuf<T> &b, const T **use)
{
    *use = src;
    if (!src || !n || in_device_memory(c, src)) return ADSB_OK;
    const int rc = grow(c, b, n);
    if (rc != ADSB_OK) return rc;
    HIPCHK(hipMemcpyAsync(b.p, src, sizeof(T) * n, hipMemcpyHostToDevice, c->aux));
    *use = b.p;
    return ADSB_OK;
}
