/* arroyo-amd device tuple-key dictionary: MI355X-native (gfx950) interner
 * for composite and nullable keys behind the arroyo_amd_tuplekey_* C ABI
 * (include/arroyo_amd.h).
 *
 * The reference keys its state on the row-encoded key tuple
 * (crates/arroyo-state/src/tables/expiring_time_key_map.rs:1008-1049): any
 * number of columns, a SQL NULL being one more key value.  Here a tuple of
 * up to AMD_TKEY_MAX_COLS 64-bit words, each with an optional Arrow
 * validity bit, is normalised once, on device, to a stable non-negative i64
 * id and the unchanged single-key engines run on the ids; decode maps ids
 * back to columns (and validity) at emission.
 *
 * Layout.  An open-addressed table of `cap` 64-bit slot words, linear
 * probing, nothing ever deleted.  The id of a tuple IS its slot index.
 *   word == 0                         empty
 *   word == tag<<32 | PENDING | 1+row claimed during this encode by batch
 *                                     row `row`; tuple still in the batch
 *   word == tag<<32 | LIVE            published; tup[slot] holds the tuple
 *   word == tag<<32 | DEAD            claimed by a call that then failed
 *                                     (capacity); matches nothing
 * tag = high 32 bits of the (possibly truncated) content hash; the home
 * slot comes from its low bits.  A tag match only selects candidates:
 * identity is always decided by the full compare of null mask and words.
 *
 * Storage is AoS: tup[slot] = {null mask, w_0 .. w_{n_cols-1}}, n_cols + 1
 * words in a row.  A probe compares, and decode gathers, whole tuples by
 * slot: AoS puts a tuple in one or two cache lines where SoA would touch
 * n_cols + 1 lines per candidate.  The word under a NULL is stored as 0 and
 * never read from the input.
 *
 * Encode is two kernels on one stream and never waits on another thread:
 *   k_tuplekey_probe    one thread per row: read words and null bits, hash,
 *                       probe.  Known tuples are a read-only lookup (plain
 *                       loads, no atomics).  An empty slot is claimed with
 *                       ONE 64-bit CAS carrying the claimer's row; a row that
 *                       meets a pending claim with its tag compares against
 *                       the claimer's row of the (immutable, already
 *                       visible) input batch, so it has its answer at once.
 *   k_tuplekey_publish  over the CAS winners only: tup[] write, pending ->
 *                       live.
 * The kernel boundary is the publish: tup[] and the live words a probe
 * kernel reads were all written by an earlier kernel.  A stale zero read of
 * a slot word is harmless (the CAS then returns the real word) and a
 * non-zero word never changes while a probe kernel runs.  Every loop is
 * bounded by the table capacity and ends in an error code.
 *
 * Validity is read as 64-bit words: blocks are 256 threads and the grid
 * stride a multiple of 256, so the 64 rows of a wave share one word per
 * column (the arrangement of update_rows<true> in updagg.hip).  Only bit r
 * of a bitmap is ever looked at for a row r < n_rows.
 */
#include <hipcub/hipcub.hpp>

#include <climits>

#include "op_common.h"

namespace tuplekey {

#define TK_PENDING 0x80000000ull
#define TK_LIVE 1ull
#define TK_DEAD 2ull

#define TKERR_CAPACITY 1
#define TKERR_BAD_ID 2
#define TKERR_RESTORE 3

#define TK_MAXC AMD_TKEY_MAX_COLS

/* device counters, re-zeroed before every call */
struct Ctr {
    int err;
    unsigned n_win;
    unsigned nullcols; /* decode: bit c = column c decoded a NULL */
    unsigned pad;
};

struct Table {
    unsigned long long *slots;
    uint64_t *tup;      /* [cap][n_cols + 1]: null mask, then the words */
    uint64_t mask;      /* cap - 1 */
    uint64_t hash_mask; /* ~0 or (1 << hash_bits) - 1 */
    int32_t n_cols;
    Ctr *ctr;
};

/* an input batch: valid[c] == nullptr marks column c all-valid */
struct Cols {
    const uint64_t *col[TK_MAXC];
    const uint64_t *valid[TK_MAXC];
};

struct OutCols {
    uint64_t *col[TK_MAXC];
    uint64_t *valid[TK_MAXC]; /* all nullptr: no validity wanted */
};

/* one tuple in registers: w[c] == 0 under a NULL and for c >= n_cols */
struct Tup {
    uint64_t w[TK_MAXC];
    unsigned nulls; /* bit c: component c is NULL */
};

__device__ __forceinline__ unsigned row_nulls(const Cols &I, int n_cols,
                                              int64_t r) {
    unsigned m = 0;
#pragma unroll
    for (int c = 0; c < TK_MAXC; c++) {
        if (c < n_cols) {
            const uint64_t *bm = I.valid[c];
            if (bm && !((bm[r >> 6] >> (r & 63)) & 1)) m |= 1u << c;
        }
    }
    return m;
}

__device__ __forceinline__ void row_load(const Cols &I, int n_cols, int64_t r,
                                         Tup &t) {
    t.nulls = row_nulls(I, n_cols, r);
#pragma unroll
    for (int c = 0; c < TK_MAXC; c++)
        t.w[c] = (c < n_cols && !((t.nulls >> c) & 1)) ? I.col[c][r] : 0;
}

/* the content hash of include/arroyo_amd.h: splitmix64 folded over the null
 * mask and the words (0 under a NULL) */
__device__ __forceinline__ uint64_t tuple_hash(const Tup &t, int n_cols) {
    uint64_t h = hash64((uint64_t)t.nulls);
#pragma unroll
    for (int c = 0; c < TK_MAXC; c++)
        if (c < n_cols) h = hash64(h ^ t.w[c]);
    return h;
}

/* is row j of the batch the tuple t?  Reads no word under a NULL. */
__device__ __forceinline__ bool row_equals(const Cols &I, int n_cols,
                                           int64_t j, const Tup &t) {
    if (row_nulls(I, n_cols, j) != t.nulls) return false;
#pragma unroll
    for (int c = 0; c < TK_MAXC; c++)
        if (c < n_cols && !((t.nulls >> c) & 1) && I.col[c][j] != t.w[c])
            return false;
    return true;
}

__device__ __forceinline__ bool slot_equals(const Table &T, uint64_t slot,
                                            const Tup &t) {
    const uint64_t *p = T.tup + slot * (uint64_t)(T.n_cols + 1);
    if (p[0] != (uint64_t)t.nulls) return false;
#pragma unroll
    for (int c = 0; c < TK_MAXC; c++)
        if (c < T.n_cols && p[1 + c] != t.w[c]) return false;
    return true;
}

__device__ __forceinline__ void slot_store(const Table &T, uint64_t slot,
                                           const Tup &t) {
    uint64_t *p = T.tup + slot * (uint64_t)(T.n_cols + 1);
    p[0] = (uint64_t)t.nulls;
#pragma unroll
    for (int c = 0; c < TK_MAXC; c++)
        if (c < T.n_cols) p[1 + c] = t.w[c];
}

__global__ void __launch_bounds__(256)
k_tuplekey_hash(Cols I, int n_cols, int64_t n_rows, uint64_t *hashes) {
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         r < n_rows; r += stride) {
        Tup t;
        row_load(I, n_cols, r, t);
        hashes[r] = tuple_hash(t, n_cols);
    }
}

__global__ void __launch_bounds__(256)
k_tuplekey_probe(Table T, Cols I, int64_t n_rows, int64_t *ids,
                 uint64_t *hashes, unsigned *win_rows) {
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         r < n_rows; r += stride) {
        Tup t;
        row_load(I, T.n_cols, r, t);
        const uint64_t full = tuple_hash(t, T.n_cols);
        if (hashes) hashes[r] = full;
        const uint64_t h = full & T.hash_mask;
        const uint64_t tag = h >> 32;
        uint64_t slot = h & T.mask;
        int64_t id = -1;
        for (uint64_t probe = 0; probe <= T.mask;
             probe++, slot = (slot + 1) & T.mask) {
            unsigned long long w = T.slots[slot];
            if (w == 0) {
                const unsigned long long mine =
                    (tag << 32) | TK_PENDING | (unsigned long long)(r + 1);
                w = atomicCAS(&T.slots[slot], 0ull, mine);
                if (w == 0) {
                    win_rows[atomicAdd(&T.ctr->n_win, 1u)] = (unsigned)r;
                    id = (int64_t)slot;
                    break;
                }
            }
            if ((w >> 32) != tag) continue;
            if (w & TK_PENDING) {
                const int64_t j = (int64_t)(w & 0x7fffffffull) - 1;
                if (row_equals(I, T.n_cols, j, t)) {
                    id = (int64_t)slot;
                    break;
                }
            } else if ((w & 0xffffffffull) == TK_LIVE) {
                if (slot_equals(T, slot, t)) {
                    id = (int64_t)slot;
                    break;
                }
            }
        }
        if (id < 0) atomicMax(&T.ctr->err, TKERR_CAPACITY);
        ids[r] = id;
    }
}

/* Winners only.  occ0 = occupied slots before this call, max_occ = the
 * load limit; a winner past the limit turns its slot DEAD. */
__global__ void __launch_bounds__(256)
k_tuplekey_publish(Table T, Cols I, const int64_t *ids,
                   const unsigned *win_rows, uint64_t occ0,
                   uint64_t max_occ) {
    const unsigned n_win = T.ctr->n_win;
    unsigned stride = gridDim.x * blockDim.x;
    for (unsigned w = blockIdx.x * blockDim.x + threadIdx.x; w < n_win;
         w += stride) {
        const int64_t r = win_rows[w];
        const int64_t slot = ids[r];
        const unsigned long long tagw =
            T.slots[slot] & 0xffffffff00000000ull;
        if (occ0 + w >= max_occ) {
            T.slots[slot] = tagw | TK_DEAD;
            atomicMax(&T.ctr->err, TKERR_CAPACITY);
            continue;
        }
        Tup t;
        row_load(I, T.n_cols, r, t);
        slot_store(T, (uint64_t)slot, t);
        T.slots[slot] = tagw | TK_LIVE;
    }
}

/* Gather ids into columns.  With validity wanted, one wave's __ballot of
 * "component c non-NULL" is the little-endian 64-bit bitmap word of its 64
 * rows; lanes past n vote 0, so the bits past n of the last word are clear.
 * An id out of range or not live is an error. */
__global__ void __launch_bounds__(256)
k_tuplekey_decode(Table T, const int64_t *ids, int64_t n, OutCols O) {
    const int lane = (int)(threadIdx.x & 63);
    const int64_t wave_id =
        ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / 64;
    const int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) / 64;
    /* wave-uniform trip count: every lane reaches every __ballot */
    for (int64_t base = wave_id * 64; base < n; base += n_waves * 64) {
        const int64_t i = base + lane;
        const bool in = i < n;
        const int64_t id = in ? ids[i] : 0;
        const bool ok = in && id >= 0 && (uint64_t)id <= T.mask &&
                        (T.slots[id] & 0xffffffffull) == TK_LIVE;
        if (in && !ok) atomicMax(&T.ctr->err, TKERR_BAD_ID);
        const uint64_t *p = T.tup + (uint64_t)(ok ? id : 0) *
                                        (uint64_t)(T.n_cols + 1);
        const unsigned nulls = ok ? (unsigned)p[0] : 0u;
#pragma unroll
        for (int c = 0; c < TK_MAXC; c++) {
            if (c < T.n_cols) {
                if (in) O.col[c][i] = ok ? p[1 + c] : 0;
                if (O.valid[c]) {
                    const unsigned long long w =
                        __ballot(in && !((nulls >> c) & 1));
                    if (lane == 0) O.valid[c][base >> 6] = w;
                }
            }
        }
        /* the flag saturates: look before joining the queue on one address */
        if (nulls & ~*(volatile unsigned *)&T.ctr->nullcols)
            atomicOr(&T.ctr->nullcols, nulls);
    }
}

/* drain: flag live slots, scan, compact their ids in slot order */
__global__ void __launch_bounds__(256)
k_tuplekey_live_flags(Table T, int64_t *flags) {
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         s <= (int64_t)T.mask; s += stride)
        flags[s] = (T.slots[s] & 0xffffffffull) == TK_LIVE;
}

__global__ void __launch_bounds__(256)
k_tuplekey_live_ids(Table T, const int64_t *flags, const int64_t *pos,
                    int64_t *ids) {
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         s <= (int64_t)T.mask; s += stride)
        if (flags[s]) ids[pos[s]] = s;
}

/* restore step 1: place every tuple at the slot its id names */
__global__ void __launch_bounds__(256)
k_tuplekey_restore_place(Table T, const int64_t *ids, Cols I,
                         int64_t n_rows) {
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         r < n_rows; r += stride) {
        const int64_t id = ids[r];
        if (id < 0 || (uint64_t)id > T.mask) {
            atomicMax(&T.ctr->err, TKERR_RESTORE);
            continue;
        }
        Tup t;
        row_load(I, T.n_cols, r, t);
        const uint64_t h = tuple_hash(t, T.n_cols) & T.hash_mask;
        const unsigned long long word = ((h >> 32) << 32) | TK_LIVE;
        if (atomicCAS(&T.slots[id], 0ull, word) != 0) { /* duplicate id */
            atomicMax(&T.ctr->err, TKERR_RESTORE);
            continue;
        }
        slot_store(T, (uint64_t)id, t);
    }
}

/* restore step 2 (next kernel, so the whole table is visible): a later
 * lookup of row r must reach slot ids[r] -- no empty slot and no equal
 * tuple on the probe path from its home slot. */
__global__ void __launch_bounds__(256)
k_tuplekey_restore_verify(Table T, const int64_t *ids, Cols I,
                          int64_t n_rows) {
    if (T.ctr->err) return;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         r < n_rows; r += stride) {
        Tup t;
        row_load(I, T.n_cols, r, t);
        const uint64_t h = tuple_hash(t, T.n_cols) & T.hash_mask;
        const uint64_t tag = h >> 32;
        uint64_t slot = h & T.mask;
        bool ok = false;
        for (uint64_t probe = 0; probe <= T.mask;
             probe++, slot = (slot + 1) & T.mask) {
            if (slot == (uint64_t)ids[r]) {
                ok = true;
                break;
            }
            const unsigned long long w = T.slots[slot];
            if (w == 0) break;
            if ((w >> 32) == tag && slot_equals(T, slot, t)) break;
        }
        if (!ok) atomicMax(&T.ctr->err, TKERR_RESTORE);
    }
}

}  // namespace tuplekey

using namespace tuplekey;

#define TK_GRID AMD_TKEY_MAX_BLOCKS

struct GpuTupleKey : OpBase {
    AmdTupleKeyConfig cfg;
    Table T;
    uint64_t cap, max_occ;
    /* host mirrors: every winner of a call occupies a slot (live or dead) */
    uint64_t n_live, occupied;
    /* per-batch scratch, grown on demand */
    unsigned *d_win;
    int64_t win_cap;
    /* host surface: staged columns and word-padded bitmaps (encode,
     * restore), gathered columns and validity words (decode, drain) */
    uint64_t *d_col[TK_MAXC], *d_bm[TK_MAXC];
    int64_t *d_ids;
    uint64_t *d_hashes;
    int64_t host_cap;
};

template <typename P>
static int tk_grow(GpuTupleKey *o, P **buf, int64_t n, size_t elem) {
    o->release(*buf);
    HIP_CHECK(o, o->dev_alloc(*buf, (size_t)n * elem));
    return 0;
}

static int64_t tk_round(int64_t have, int64_t want) {
    int64_t n = have ? have : 1024;
    while (n < want) n *= 2;
    return n;
}

static int tk_reserve_win(GpuTupleKey *o, int64_t n_rows) {
    if (n_rows <= o->win_cap) return 0;
    /* allocations belong on the handle's device, whatever the caller's
     * current one is */
    HIP_CHECK(o, hipSetDevice(o->cfg.device));
    const int64_t n = tk_round(o->win_cap, n_rows);
    o->win_cap = 0;
    if (tk_grow(o, &o->d_win, n, sizeof(unsigned))) return 1;
    o->win_cap = n;
    return 0;
}

/* the host surface's buffers for n_rows rows: a multiple of 64 rows, so a
 * bitmap buffer is whole 64-bit words */
static int tk_reserve_host(GpuTupleKey *o, int64_t n_rows) {
    if (n_rows <= o->host_cap) return 0;
    HIP_CHECK(o, hipSetDevice(o->cfg.device));
    const int64_t n = tk_round(o->host_cap, n_rows);
    o->host_cap = 0;
    for (int c = 0; c < o->cfg.n_cols; c++) {
        if (tk_grow(o, &o->d_col[c], n, 8)) return 1;
        if (o->cfg.nullable && tk_grow(o, &o->d_bm[c], n / 64, 8)) return 1;
    }
    if (tk_grow(o, &o->d_ids, n, 8)) return 1;
    if (tk_grow(o, &o->d_hashes, n, 8)) return 1;
    o->host_cap = n;
    return 0;
}

API void *arroyo_amd_tuplekey_create(const AmdTupleKeyConfig *cfg) {
    if (!cfg) {
        snprintf(g_create_err, sizeof g_create_err,
                 "invalid tuplekey config: null");
        return nullptr;
    }
    if (cfg->n_cols < 1 || cfg->n_cols > AMD_TKEY_MAX_COLS) {
        snprintf(g_create_err, sizeof g_create_err,
                 "invalid tuplekey config: n_cols %d (1..%d)", cfg->n_cols,
                 AMD_TKEY_MAX_COLS);
        return nullptr;
    }
    if (cfg->log2_capacity < 1 || cfg->log2_capacity > 30) {
        snprintf(g_create_err, sizeof g_create_err,
                 "invalid tuplekey config: log2_capacity %d (1..30)",
                 cfg->log2_capacity);
        return nullptr;
    }
    if (cfg->hash_bits < 0 || cfg->hash_bits > 63) {
        snprintf(g_create_err, sizeof g_create_err,
                 "invalid tuplekey config: hash_bits %d (0..63)",
                 cfg->hash_bits);
        return nullptr;
    }
    if (cfg->nullable != 0 && cfg->nullable != 1) {
        snprintf(g_create_err, sizeof g_create_err,
                 "invalid tuplekey config: nullable %d (0 or 1)",
                 cfg->nullable);
        return nullptr;
    }
    if (hipSetDevice(cfg->device) != hipSuccess) {
        snprintf(g_create_err, sizeof g_create_err,
                 "hipSetDevice(%d) failed: no HIP device (no CPU fallback)",
                 cfg->device);
        return nullptr;
    }
    GpuTupleKey *o = new GpuTupleKey();
    o->cfg = *cfg;
    o->cap = 1ull << cfg->log2_capacity;
    /* load limit 7/8: keeps a free slot on every probe path */
    o->max_occ = o->cap - o->cap / 8;
    o->T.mask = o->cap - 1;
    o->T.hash_mask = cfg->hash_bits ? (1ull << cfg->hash_bits) - 1 : ~0ull;
    o->T.n_cols = cfg->n_cols;
    OP_TRY(o, "tuplekey alloc", o->dev_alloc(o->T.slots, o->cap * 8, 0));
    OP_TRY(o, "tuplekey alloc",
           o->dev_alloc(o->T.tup, o->cap * 8 * (size_t)(cfg->n_cols + 1)));
    OP_TRY(o, "tuplekey alloc", o->dev_alloc(o->T.ctr, sizeof(Ctr), 0));
    OP_TRY(o, "tuplekey alloc", o->stream_create(&o->stream));
    return o;
}

API const char *arroyo_amd_tuplekey_last_error(void *h) {
    return h ? ((GpuTupleKey *)h)->err_msg : g_create_err;
}

API void arroyo_amd_tuplekey_destroy(void *h) {
    delete (GpuTupleKey *)h;   /* ~OpBase drains the stream first */
}

static int tk_zero_counters(GpuTupleKey *o) {
    HIP_CHECK(o, hipMemsetAsync(o->T.ctr, 0, sizeof(Ctr), o->stream));
    return 0;
}

/* read the counters back; synchronises the stream */
static int tk_sync_counters(GpuTupleKey *o, Ctr *c) {
    HIP_CHECK(o, hipMemcpyAsync(c, o->T.ctr, sizeof(Ctr),
                                hipMemcpyDeviceToHost, o->stream));
    HIP_CHECK(o, hipStreamSynchronize(o->stream));
    return 0;
}

static int tk_report(GpuTupleKey *o, int err) {
    switch (err) {
    case 0:
        return 0;
    case TKERR_CAPACITY:
        snprintf(o->err_msg, sizeof o->err_msg,
                 "tuple dictionary capacity exhausted: %llu of %llu slots in "
                 "use (limit %llu); raise log2_capacity",
                 (unsigned long long)o->occupied, (unsigned long long)o->cap,
                 (unsigned long long)o->max_occ);
        break;
    case TKERR_BAD_ID:
        snprintf(o->err_msg, sizeof o->err_msg,
                 "decode of an id this dictionary never issued");
        break;
    default:
        snprintf(o->err_msg, sizeof o->err_msg,
                 "restore: an id is out of range, duplicated or not "
                 "reachable from its tuple's home slot (n_cols, "
                 "log2_capacity, hash_bits and nullable must match the "
                 "drained handle)");
    }
    return 1;
}

/* 0 rows: *empty = 1 and success; otherwise the per-call row limit (the
 * claim word carries 1 + row in 31 bits) */
static int tk_check_rows(GpuTupleKey *o, int64_t n_rows, int *empty) {
    *empty = n_rows == 0;
    if (n_rows < 0) {
        snprintf(o->err_msg, sizeof o->err_msg, "invalid n_rows %lld",
                 (long long)n_rows);
        return 1;
    }
    if (n_rows > (int64_t)INT32_MAX - 1) {
        snprintf(o->err_msg, sizeof o->err_msg,
                 "n_rows %lld is over the limit of %d rows per call",
                 (long long)n_rows, INT32_MAX - 1);
        return 1;
    }
    return 0;
}

/* a bitmap on a nullable = 0 handle is an error; on the device surface a
 * bitmap is read as 64-bit words and must be aligned for that */
static int tk_check_validity(GpuTupleKey *o, const uint8_t *const *validity,
                             bool device) {
    for (int c = 0; validity && c < o->cfg.n_cols; c++) {
        if (!validity[c]) continue;
        if (!o->cfg.nullable) {
            snprintf(o->err_msg, sizeof o->err_msg,
                     "validity bitmap on column %d of a handle created with "
                     "nullable = 0", c);
            return 1;
        }
        if (device && ((uintptr_t)validity[c] & 7)) {
            snprintf(o->err_msg, sizeof o->err_msg,
                     "device validity bitmap of column %d is not 8-byte "
                     "aligned", c);
            return 1;
        }
    }
    return 0;
}

static void tk_device_cols(GpuTupleKey *o, const void *const *d_cols,
                           const uint8_t *const *d_validity, Cols *I) {
    memset(I, 0, sizeof *I);
    for (int c = 0; c < o->cfg.n_cols; c++) {
        I->col[c] = (const uint64_t *)d_cols[c];
        if (d_validity) I->valid[c] = (const uint64_t *)d_validity[c];
    }
}

/* Host columns and bitmaps -> the handle's staging buffers.  A bitmap is
 * copied as its (n_rows + 7) / 8 bytes into a buffer of whole words, so no
 * read goes past the caller's allocation. */
static int tk_stage(GpuTupleKey *o, const void *const *cols,
                    const uint8_t *const *validity, int64_t n_rows, Cols *I) {
    if (tk_reserve_host(o, n_rows)) return 1;
    memset(I, 0, sizeof *I);
    const size_t nbytes = (size_t)((n_rows + 7) / 8);
    const size_t nwords = (size_t)((n_rows + 63) / 64);
    for (int c = 0; c < o->cfg.n_cols; c++) {
        HIP_CHECK(o, hipMemcpyAsync(o->d_col[c], cols[c], (size_t)n_rows * 8,
                                    hipMemcpyHostToDevice, o->stream));
        I->col[c] = o->d_col[c];
        if (!validity || !validity[c]) continue;
        HIP_CHECK(o, hipMemsetAsync(o->d_bm[c] + (nwords - 1), 0, 8,
                                    o->stream));
        HIP_CHECK(o, hipMemcpyAsync(o->d_bm[c], validity[c], nbytes,
                                    hipMemcpyHostToDevice, o->stream));
        I->valid[c] = o->d_bm[c];
    }
    return 0;
}

/* the encode core: columns, bitmaps and outputs all on the device */
static int tk_encode_core(GpuTupleKey *o, const Cols &I, int64_t n_rows,
                          int64_t *d_ids, uint64_t *d_hashes) {
    if (tk_reserve_win(o, n_rows)) return 1;
    if (tk_zero_counters(o)) return 1;
    hipLaunchKernelGGL(k_tuplekey_probe, dim3(grid_for(n_rows, TK_GRID)),
                       dim3(AMD_TKEY_BLOCK_THREADS), 0, o->stream, o->T, I,
                       n_rows, d_ids, d_hashes, o->d_win);
    hipLaunchKernelGGL(k_tuplekey_publish, dim3(256),
                       dim3(AMD_TKEY_BLOCK_THREADS), 0, o->stream, o->T, I,
                       (const int64_t *)d_ids, (const unsigned *)o->d_win,
                       o->occupied, o->max_occ);
    HIP_CHECK(o, hipGetLastError());
    Ctr c;
    if (tk_sync_counters(o, &c)) return 1;
    const uint64_t room = o->max_occ - std::min(o->max_occ, o->occupied);
    o->n_live += std::min<uint64_t>(c.n_win, room);
    o->occupied += c.n_win;
    return tk_report(o, c.err);
}

API int arroyo_amd_tuplekey_encode_device(void *h, const void *const *d_cols,
                                          const uint8_t *const *d_validity,
                                          int64_t n_rows, int64_t *d_ids_out,
                                          uint64_t *d_hashes_out) {
    GpuTupleKey *o = (GpuTupleKey *)h;
    int empty;
    if (tk_check_rows(o, n_rows, &empty)) return 1;
    if (empty) return 0;
    if (tk_check_validity(o, d_validity, true)) return 1;
    Cols I;
    tk_device_cols(o, d_cols, d_validity, &I);
    return tk_encode_core(o, I, n_rows, d_ids_out, d_hashes_out);
}

API int arroyo_amd_tuplekey_encode(void *h, const void *const *cols,
                                   const uint8_t *const *validity,
                                   int64_t n_rows, int64_t *ids_out,
                                   uint64_t *hashes_out) {
    GpuTupleKey *o = (GpuTupleKey *)h;
    int empty;
    if (tk_check_rows(o, n_rows, &empty)) return 1;
    if (empty) return 0;
    if (tk_check_validity(o, validity, false)) return 1;
    Cols I;
    if (tk_stage(o, cols, validity, n_rows, &I)) return 1;
    if (tk_encode_core(o, I, n_rows, o->d_ids,
                       hashes_out ? o->d_hashes : nullptr))
        return 1;
    HIP_CHECK(o, hipMemcpyAsync(ids_out, o->d_ids, (size_t)n_rows * 8,
                                hipMemcpyDeviceToHost, o->stream));
    if (hashes_out)
        HIP_CHECK(o, hipMemcpyAsync(hashes_out, o->d_hashes,
                                    (size_t)n_rows * 8, hipMemcpyDeviceToHost,
                                    o->stream));
    HIP_CHECK(o, hipStreamSynchronize(o->stream));
    return 0;
}

API int arroyo_amd_tuplekey_hash_device(void *h, const void *const *d_cols,
                                        const uint8_t *const *d_validity,
                                        int64_t n_rows,
                                        uint64_t *d_hashes_out) {
    GpuTupleKey *o = (GpuTupleKey *)h;
    int empty;
    if (tk_check_rows(o, n_rows, &empty)) return 1;
    if (empty) return 0;
    if (tk_check_validity(o, d_validity, true)) return 1;
    Cols I;
    tk_device_cols(o, d_cols, d_validity, &I);
    hipLaunchKernelGGL(k_tuplekey_hash, dim3(grid_for(n_rows, TK_GRID)),
                       dim3(AMD_TKEY_BLOCK_THREADS), 0, o->stream, I,
                       o->cfg.n_cols, n_rows, d_hashes_out);
    HIP_CHECK(o, hipGetLastError());
    HIP_CHECK(o, hipStreamSynchronize(o->stream));
    return 0;
}

/* launch the gather of n device-resident ids and read the counters back */
static int tk_decode_core(GpuTupleKey *o, const int64_t *d_ids, int64_t n,
                          const OutCols &O, Ctr *c) {
    if (tk_zero_counters(o)) return 1;
    hipLaunchKernelGGL(k_tuplekey_decode, dim3(grid_for(n, TK_GRID)),
                       dim3(AMD_TKEY_BLOCK_THREADS), 0, o->stream, o->T,
                       d_ids, n, O);
    HIP_CHECK(o, hipGetLastError());
    if (tk_sync_counters(o, c)) return 1;
    return tk_report(o, c->err);
}

API int arroyo_amd_tuplekey_decode_device(void *h, const int64_t *d_ids,
                                          int64_t n_rows,
                                          void *const *d_cols_out,
                                          uint64_t *const *d_validity_out) {
    GpuTupleKey *o = (GpuTupleKey *)h;
    int empty;
    if (tk_check_rows(o, n_rows, &empty)) return 1;
    if (!o->cfg.nullable && d_validity_out) {
        snprintf(o->err_msg, sizeof o->err_msg,
                 "validity output on a handle created with nullable = 0");
        return 1;
    }
    if (o->cfg.nullable && !d_validity_out) {
        snprintf(o->err_msg, sizeof o->err_msg,
                 "decode_device on a nullable handle needs d_validity_out");
        return 1;
    }
    if (empty) return 0;
    OutCols O = {};
    for (int c = 0; c < o->cfg.n_cols; c++) {
        O.col[c] = (uint64_t *)d_cols_out[c];
        if (!d_validity_out) continue;
        if (!d_validity_out[c] || ((uintptr_t)d_validity_out[c] & 7)) {
            snprintf(o->err_msg, sizeof o->err_msg,
                     "d_validity_out[%d] is NULL or not 8-byte aligned", c);
            return 1;
        }
        O.valid[c] = d_validity_out[c];
    }
    Ctr c;
    return tk_decode_core(o, d_ids, n_rows, O, &c);
}

/* Decode n device-resident ids into a host batch of first_col + n_cols
 * columns (the components from column first_col on); a validity table only
 * if some component is NULL, a bitmap only for the columns that have one.
 * On an error the batch is freed. */
static int tk_decode_to_host(GpuTupleKey *o, const int64_t *d_ids, int64_t n,
                             int first_col, AmdOutBatch *out,
                             const char *who) {
    if (tk_reserve_host(o, n)) return 1;
    OutCols O = {};
    for (int c = 0; c < o->cfg.n_cols; c++) {
        O.col[c] = o->d_col[c];
        if (o->cfg.nullable) O.valid[c] = o->d_bm[c];
    }
    Ctr ctr;
    if (tk_decode_core(o, d_ids, n, O, &ctr)) return 1;
    if (op_out_alloc(o, out, n, first_col + o->cfg.n_cols, who)) return 1;
    hipError_t e = hipSuccess;
    for (int c = 0; c < o->cfg.n_cols && e == hipSuccess; c++)
        e = hipMemcpyAsync(out->cols[first_col + c], o->d_col[c],
                           (size_t)n * 8, hipMemcpyDeviceToHost, o->stream);
    if (e == hipSuccess && ctr.nullcols) {
        if (out_alloc_validity(out)) {
            out_free_host(out);
            snprintf(o->err_msg, sizeof o->err_msg,
                     "%s: validity bitmap table allocation failed", who);
            return 1;
        }
        for (int c = 0; c < o->cfg.n_cols && e == hipSuccess; c++) {
            if (!((ctr.nullcols >> c) & 1)) continue;
            uint8_t *bm = out_validity_col(out, first_col + c);
            if (!bm) {
                out_free_host(out);
                snprintf(o->err_msg, sizeof o->err_msg,
                         "%s: validity bitmap allocation failed", who);
                return 1;
            }
            e = hipMemcpyAsync(bm, o->d_bm[c], (size_t)((n + 7) / 8),
                               hipMemcpyDeviceToHost, o->stream);
        }
    }
    if (e == hipSuccess) e = hipStreamSynchronize(o->stream);
    if (e != hipSuccess) out_free_host(out);
    HIP_CHECK(o, e);
    return 0;
}

API int arroyo_amd_tuplekey_decode(void *h, const int64_t *ids,
                                   int64_t n_rows, AmdOutBatch *out) {
    GpuTupleKey *o = (GpuTupleKey *)h;
    memset(out, 0, sizeof *out);
    int empty;
    if (tk_check_rows(o, n_rows, &empty)) return 1;
    if (empty)
        return op_out_alloc(o, out, 0, o->cfg.n_cols, "tuplekey_decode");
    if (tk_reserve_host(o, n_rows)) return 1;
    HIP_CHECK(o, hipMemcpyAsync(o->d_ids, ids, (size_t)n_rows * 8,
                                hipMemcpyHostToDevice, o->stream));
    return tk_decode_to_host(o, o->d_ids, n_rows, 0, out, "tuplekey_decode");
}

API int arroyo_amd_tuplekey_count(void *h, int64_t *n_tuples) {
    GpuTupleKey *o = (GpuTupleKey *)h;
    if (n_tuples) *n_tuples = (int64_t)o->n_live;
    return 0;
}

API int arroyo_amd_tuplekey_checkpoint_drain(void *h, AmdOutBatch *out) {
    GpuTupleKey *o = (GpuTupleKey *)h;
    const char *who = "tuplekey_checkpoint_drain";
    memset(out, 0, sizeof *out);
    const int64_t n = (int64_t)o->n_live;
    if (n == 0) return op_out_alloc(o, out, 0, 1 + o->cfg.n_cols, who);
    const int64_t cap = (int64_t)o->cap;
    HIP_CHECK(o, hipSetDevice(o->cfg.device));
    DevScratch t;
    int64_t *flags = nullptr, *pos = nullptr, *ids = nullptr;
    void *cub = nullptr;
    HIP_CHECK(o, t.alloc(flags, (size_t)cap * 8));
    HIP_CHECK(o, t.alloc(pos, (size_t)cap * 8));
    HIP_CHECK(o, t.alloc(ids, (size_t)n * 8));
    size_t cub_bytes = 0;
    HIP_CHECK(o, hipcub::DeviceScan::ExclusiveSum(nullptr, cub_bytes, flags,
                                                  pos, (int)cap));
    HIP_CHECK(o, t.alloc(cub, cub_bytes ? cub_bytes : 1));
    const int grid = grid_for(cap, TK_GRID);
    hipLaunchKernelGGL(k_tuplekey_live_flags, dim3(grid), dim3(256), 0,
                       o->stream, o->T, flags);
    HIP_CHECK(o, hipcub::DeviceScan::ExclusiveSum(cub, cub_bytes, flags, pos,
                                                  (int)cap, o->stream));
    hipLaunchKernelGGL(k_tuplekey_live_ids, dim3(grid), dim3(256), 0,
                       o->stream, o->T, (const int64_t *)flags,
                       (const int64_t *)pos, ids);
    HIP_CHECK(o, hipGetLastError());
    if (tk_decode_to_host(o, ids, n, 1, out, who)) return 1;
    hipError_t e = hipMemcpyAsync(out->cols[0], ids, (size_t)n * 8,
                                  hipMemcpyDeviceToHost, o->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(o->stream);
    if (e != hipSuccess) out_free_host(out);
    HIP_CHECK(o, e);
    return 0;
}

API int arroyo_amd_tuplekey_restore(void *h, const int64_t *ids,
                                    const void *const *cols,
                                    const uint8_t *const *validity,
                                    int64_t n_rows) {
    GpuTupleKey *o = (GpuTupleKey *)h;
    if (o->occupied != 0) {
        snprintf(o->err_msg, sizeof o->err_msg,
                 "restore into a non-empty dictionary (%llu tuples held)",
                 (unsigned long long)o->n_live);
        return 1;
    }
    int empty;
    if (tk_check_rows(o, n_rows, &empty)) return 1;
    if (empty) return 0;
    if ((uint64_t)n_rows > o->max_occ) {
        snprintf(o->err_msg, sizeof o->err_msg,
                 "restore of %lld tuples exceeds the dictionary capacity "
                 "(limit %llu of %llu slots; log2_capacity must match the "
                 "drained handle)",
                 (long long)n_rows, (unsigned long long)o->max_occ,
                 (unsigned long long)o->cap);
        return 1;
    }
    if (tk_check_validity(o, validity, false)) return 1;
    Cols I;
    if (tk_stage(o, cols, validity, n_rows, &I)) return 1;
    HIP_CHECK(o, hipMemcpyAsync(o->d_ids, ids, (size_t)n_rows * 8,
                                hipMemcpyHostToDevice, o->stream));
    if (tk_zero_counters(o)) return 1;
    const int grid = grid_for(n_rows, TK_GRID);
    hipLaunchKernelGGL(k_tuplekey_restore_place, dim3(grid), dim3(256), 0,
                       o->stream, o->T, (const int64_t *)o->d_ids, I, n_rows);
    hipLaunchKernelGGL(k_tuplekey_restore_verify, dim3(grid), dim3(256), 0,
                       o->stream, o->T, (const int64_t *)o->d_ids, I, n_rows);
    HIP_CHECK(o, hipGetLastError());
    Ctr c;
    if (tk_sync_counters(o, &c)) return 1;
    if (c.err) {
        /* a failed restore leaves the handle empty, not half loaded */
        int rc = tk_report(o, c.err);
        HIP_CHECK(o, hipMemsetAsync(o->T.slots, 0, o->cap * 8, o->stream));
        HIP_CHECK(o, hipStreamSynchronize(o->stream));
        return rc;
    }
    o->n_live = o->occupied = (uint64_t)n_rows;
    return 0;
}
