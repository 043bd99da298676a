/* What every operator file (*.hip) shares: the device hash/table helpers,
 * the owning base of an operator handle, the HIP check macro, host-ingest
 * staging, launch-grid clamp, device-error readback and the D2H half of an
 * output batch.  A new operator starts from this header (DESIGN.md,
 * "Shared operator base"). */
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "op_out.h"

#define API extern "C" __attribute__((visibility("default")))

/* ------------------------------------------------------------------ */
/* device side                                                         */

#define EMPTY_KEY  (-1LL)          /* all-0xFF bytes: memset-clearable */
#define EMPTY_TAG  (~0ULL)
#define ERR_TABLE_FULL    3

__device__ inline uint64_t hash64(uint64_t x) {
    x += 0x9e3779b97f4a7c15ULL;
    x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ULL;
    x = (x ^ (x >> 27)) * 0x94d049bb133111ebULL;
    return x ^ (x >> 31);
}

/* claim-or-find a key slot in an open-addressing table.
 * Keys transition EMPTY->k exactly once, so the plain-load fast path is
 * safe: a stale L1 read can only see EMPTY, and the CAS resolves it.
 * Fullness is detected by probe length (expected probe count at <=7/8 load
 * is single digits; a 256-probe chain means the table is effectively full).
 * No per-insert fill counter: a same-address atomicAdd per insert was
 * serializing at the L2 bank. */
#define MAX_PROBES 256u

__device__ inline int64_t table_upsert(int64_t *keys, uint32_t C, int64_t key,
                                       int *err) {
    uint64_t m = C - 1;
    uint64_t i = hash64((uint64_t)key) & m;
    uint32_t lim = C < MAX_PROBES ? C : MAX_PROBES;
    for (uint32_t probes = 0; probes < lim; probes++) {
        int64_t k = keys[i];
        if (k == key) return (int64_t)i;
        if (k == EMPTY_KEY) {
            int64_t old = (int64_t)atomicCAS((unsigned long long *)&keys[i],
                                             (unsigned long long)EMPTY_KEY,
                                             (unsigned long long)key);
            if (old == EMPTY_KEY || old == key) return (int64_t)i;
        }
        i = (i + 1) & m;
    }
    *err = ERR_TABLE_FULL;
    return -1;
}

/* order-preserving f64 <-> u64 with the all-zero bit pattern as identity:
 * flip maps ordered (non-NaN) doubles onto (0x000F.., 0xFFF0..] of u64, so
 * a memset-zero state is below every real encoding (MAX) and, negated,
 * above every real one (MIN) — same memset-retirable property as the i64
 * encodes.  Over all bit patterns the order is IEEE totalOrder (-NaN < -inf
 * < ... < -0.0 < +0.0 < ... < +inf < +NaN, NaNs by payload), and the zero
 * state decodes to the one NaN pattern whose encoding is 0 (0xFFFF..FF for
 * MAX, 0x7FFF..FF for MIN), so every pattern round-trips. */
__host__ __device__ inline uint64_t f64flip(uint64_t b) {
    return (b & 0x8000000000000000ULL) ? ~b : (b | 0x8000000000000000ULL);
}
__host__ __device__ inline uint64_t f64unflip(uint64_t e) {
    return (e & 0x8000000000000000ULL) ? (e & ~0x8000000000000000ULL) : ~e;
}
__host__ __device__ inline uint64_t enc_minf(int64_t bits) {
    return ~f64flip((uint64_t)bits);
}
__host__ __device__ inline int64_t dec_minf(uint64_t e) {
    return (int64_t)f64unflip(~e);
}
__host__ __device__ inline uint64_t enc_maxf(int64_t bits) {
    return f64flip((uint64_t)bits);
}
__host__ __device__ inline int64_t dec_maxf(uint64_t e) {
    return (int64_t)f64unflip(e);
}

/* ------------------------------------------------------------------ */
/* host side                                                           */

/* create-time errors, before a handle exists: what every
 * *_last_error(NULL) returns */
inline thread_local char g_create_err[512];

/* run a HIP call from a function returning int; on failure leave
 * "file:line hip: <error>" in the handle's err_msg and return 1 */
#define HIP_CHECK(o, call)                                                    \
    do {                                                                      \
        hipError_t _e = (call);                                               \
        if (_e != hipSuccess) {                                               \
            snprintf((o)->err_msg, sizeof (o)->err_msg, "%s:%d hip: %s",      \
                     __FILE__, __LINE__, hipGetErrorString(_e));              \
            return 1;                                                         \
        }                                                                     \
    } while (0)

/* Owning base of an operator handle.  Every device and pinned buffer, extra
 * stream and event of the handle's lifetime is taken through it, so the
 * destructor is the one place that gives them back: a failed create and
 * destroy are both `delete o`.  Handles are created with `new T()`, which
 * zero-fills the plain members below and the derived struct's. */
struct OpBase {
    hipStream_t stream;
    char err_msg[512];
    int *d_err;
    std::vector<void *> dev_bufs, pinned_bufs;
    std::vector<hipStream_t> streams;
    std::vector<hipEvent_t> events;

    /* fill >= 0: set every byte of the new buffer to it.  The fill is a
     * synchronous hipMemset on the NULL stream: right at create, and
     * mid-life only for a handle whose stream is a blocking one
     * (hipStreamCreate), which the NULL stream orders with.  The window
     * operator's streams are hipStreamNonBlocking: mid-life it must fill
     * with hipMemsetAsync on its own stream instead. */
    template <class T>
    hipError_t dev_alloc(T *&p, size_t bytes, int fill = -1) {
        void *q = nullptr;
        hipError_t e = hipMalloc(&q, bytes);
        if (e != hipSuccess) return e;
        if (q) dev_bufs.push_back(q);
        p = (T *)q;
        return fill >= 0 && q ? hipMemset(q, fill, bytes) : hipSuccess;
    }
    template <class T>
    hipError_t pinned_alloc(T *&p, size_t bytes) {
        void *q = nullptr;
        hipError_t e = hipHostMalloc(&q, bytes);
        if (e != hipSuccess) return e;
        if (q) pinned_bufs.push_back(q);
        p = (T *)q;
        return hipSuccess;
    }
    /* register a stream some hipStreamCreate* flavour just made:
     * own_stream(s, hipStreamCreateWithPriority(&s, ...)) */
    hipError_t own_stream(hipStream_t &s, hipError_t e) {
        if (e == hipSuccess) streams.push_back(s);
        return e;
    }
    hipError_t stream_create(hipStream_t *s) {
        return own_stream(*s, hipStreamCreate(s));
    }
    hipError_t event_create(hipEvent_t *ev, unsigned flags = hipEventDefault) {
        hipError_t e = hipEventCreateWithFlags(ev, flags);
        if (e == hipSuccess) events.push_back(*ev);
        return e;
    }
    /* give back one buffer early (regrown or rebuilt mid-life) */
    template <class T>
    void release(T *&p) {
        for (auto *v : {&dev_bufs, &pinned_bufs}) {
            auto it = std::find(v->begin(), v->end(), (void *)p);
            if (it == v->end()) continue;
            (void)(v == &dev_bufs ? hipFree(*it) : hipHostFree(*it));
            v->erase(it);
        }
        p = nullptr;
    }
    /* drain the handle's streams, then give back events, buffers and the
     * streams themselves */
    ~OpBase() {
        for (hipStream_t s : streams) (void)hipStreamSynchronize(s);
        for (hipEvent_t ev : events) (void)hipEventDestroy(ev);
        for (void *p : dev_bufs) (void)hipFree(p);
        for (void *p : pinned_bufs) (void)hipHostFree(p);
        for (hipStream_t s : streams) (void)hipStreamDestroy(s);
    }
};

/* a create that cannot finish: message for *_last_error(NULL), then the
 * handle's destructor returns everything taken so far */
template <class T>
void *create_fail(T *o, const char *what, hipError_t e) {
    snprintf(g_create_err, sizeof g_create_err, "%s: %s", what,
             hipGetErrorString(e));
    delete o;
    return nullptr;
}

/* the same with a fixed message */
template <class T>
void *create_fail(T *o, const char *msg) {
    snprintf(g_create_err, sizeof g_create_err, "%s", msg);
    delete o;
    return nullptr;
}

/* create-time steps (in a function returning the handle as void *):
 * OP_TRY reports "<what>: <hip error>", OP_TRY_MSG the message alone */
#define OP_TRY(o, what, call)                                                 \
    do {                                                                      \
        hipError_t _e = (call);                                               \
        if (_e != hipSuccess) return create_fail(o, what, _e);                \
    } while (0)
#define OP_TRY_MSG(o, msg, call)                                              \
    do {                                                                      \
        if ((call) != hipSuccess) return create_fail(o, msg);                 \
    } while (0)
/* OP_ALLOC(o, ptr, bytes[, fill byte]) */
#define OP_ALLOC(o, p, ...) OP_TRY(o, #p, (o)->dev_alloc(p, __VA_ARGS__))

/* Device scratch of one call (restore paths): freed when it goes out of
 * scope, on the error returns too.  Not for handle-lifetime buffers. */
struct DevScratch {
    std::vector<void *> bufs;
    template <class T>
    hipError_t alloc(T *&p, size_t bytes) {
        void *q = nullptr;
        hipError_t e = hipMalloc(&q, bytes);
        if (e == hipSuccess && q) bufs.push_back(q);
        p = (T *)q;
        return e;
    }
    /* device copy of n host elements */
    template <class T>
    hipError_t upload(T *&p, const T *src, size_t n) {
        hipError_t e = alloc(p, n * sizeof(T));
        if (e != hipSuccess) return e;
        return hipMemcpy(p, src, n * sizeof(T), hipMemcpyHostToDevice);
    }
    ~DevScratch() {
        for (void *p : bufs) (void)hipFree(p);
    }
};

/* Host-ingest staging: pinned host columns and their device twins, `cap`
 * rows each.  `n` counts rows gathered in h[] and not yet uploaded, for
 * callers that accumulate across calls. */
#define OP_STG_MAX_COLS 32
struct Staging {
    int64_t *h[OP_STG_MAX_COLS], *d[OP_STG_MAX_COLS];
    int64_t cap, n;

    hipError_t alloc(OpBase *o, int ncols, int64_t rows) {
        cap = rows;
        n = 0;
        hipError_t e = hipSuccess;
        for (int c = 0; c < ncols && e == hipSuccess; c++) {
            e = o->pinned_alloc(h[c], (size_t)rows * 8);
            if (e == hipSuccess) e = o->dev_alloc(d[c], (size_t)rows * 8);
        }
        return e;
    }
    /* H2D of the first `rows` rows of h[c] on the owner's stream;
     * dcols[c] = the device twin */
    int upload_col(OpBase *o, int c, int64_t rows, const int64_t **dcols) {
        HIP_CHECK(o, hipMemcpyAsync(d[c], h[c], (size_t)rows * 8,
                                    hipMemcpyHostToDevice, o->stream));
        dcols[c] = d[c];
        return 0;
    }
    int upload(OpBase *o, int ncols, int64_t rows, const int64_t **dcols) {
        for (int c = 0; c < ncols; c++)
            if (upload_col(o, c, rows, dcols)) return 1;
        return 0;
    }
    /* rows [done, done + take) of the caller's host columns -> device; each
     * column's copy is in flight while the next one is staged */
    int stage_chunk(OpBase *o, const int64_t *const *cols, int ncols,
                    int64_t done, int64_t take, const int64_t **dcols) {
        for (int c = 0; c < ncols; c++) {
            memcpy(h[c], cols[c] + done, (size_t)take * 8);
            if (upload_col(o, c, take, dcols)) return 1;
        }
        return 0;
    }
};

/* blocks of 256 threads for `want_threads`, clamped to [1, max_blocks] */
static inline int grid_for(int64_t want_threads, int max_blocks) {
    int64_t w = (want_threads + 255) / 256;
    return (int)(w > max_blocks ? max_blocks : (w < 1 ? 1 : w));
}

/* read the device error word on the operator's stream (syncs it); nonzero
 * code -> msg_fn's message in err_msg, return 1 */
static inline int op_check_err(OpBase *o, const char *(*msg_fn)(int)) {
    int e = 0;
    HIP_CHECK(o, hipMemcpyAsync(&e, o->d_err, 4, hipMemcpyDeviceToHost,
                                o->stream));
    HIP_CHECK(o, hipStreamSynchronize(o->stream));
    if (!e) return 0;
    snprintf(o->err_msg, sizeof o->err_msg, "%s", msg_fn(e));
    return 1;
}

/* out_alloc with the library's loud-error convention: on failure `out` is
 * zeroed and err_msg says which function could not allocate */
static inline int op_out_alloc(OpBase *o, AmdOutBatch *out, int64_t n_rows,
                               int n_cols, const char *who) {
    if (!out_alloc(out, n_rows, n_cols)) return 0;
    snprintf(o->err_msg, sizeof o->err_msg, "%s: host allocation failed", who);
    return 1;
}

/* first n rows of each device column -> the allocated host batch, then one
 * sync; frees the batch on a HIP error */
static inline int out_copy_cols(OpBase *o, AmdOutBatch *out,
                                const int64_t *const *d_cols, int64_t n) {
    hipError_t e = hipSuccess;
    for (int i = 0; n && i < out->n_cols && e == hipSuccess; i++)
        e = hipMemcpyAsync(out->cols[i], d_cols[i], (size_t)n * 8,
                           hipMemcpyDeviceToHost, o->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(o->stream);
    if (e != hipSuccess) out_free_host(out);
    HIP_CHECK(o, e);
    return 0;
}
