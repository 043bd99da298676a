/* arroyo-amd device string-key dictionary: MI355X-native (gfx950) interner
 * for Arrow Utf8 key columns behind the arroyo_amd_strkey_* C ABI
 * (include/arroyo_amd.h).
 *
 * The reference keys its state on arbitrary Arrow types by row-encoding the
 * key tuple (crates/arroyo-state/src/tables/expiring_time_key_map.rs
 * :1008-1049).  Here a string key is normalised once, on device, to a stable
 * non-negative i64 id and the unchanged single-key engines run on the ids;
 * decode maps ids back to strings at emission.
 *
 * Layout.  An open-addressed table of `cap` 64-bit slot words, linear
 * probing, nothing ever deleted.  The id of a string IS its slot index.
 *   word == 0                         empty
 *   word == tag<<32 | PENDING | 1+row claimed during this encode by batch
 *                                     row `row`; bytes still in the batch
 *   word == tag<<32 | LIVE            published; ent[slot] = {arena off, len}
 *   word == tag<<32 | DEAD            claimed by a call that then failed
 *                                     (arena/capacity); matches nothing
 * tag = high 32 bits of the (possibly truncated) content hash; the home
 * slot comes from its low bits.  A tag match only selects candidates:
 * identity is always decided by a full length-and-bytes compare.
 *
 * Encode is two kernels on one stream and never waits on another thread:
 *   k_strkey_probe    one thread per row: hash, probe.  Known strings are a
 *                     read-only lookup (plain loads, no atomics).  An empty
 *                     slot is claimed with ONE 64-bit CAS carrying the
 *                     claimer's row; a row that meets a pending claim with
 *                     its tag compares against the claimer's bytes in the
 *                     (immutable, already visible) input batch, so it has
 *                     its answer at once.
 *   k_strkey_publish  over the CAS winners only: arena space by one atomic
 *                     add, byte copy, ent[] write, pending -> live.
 * The kernel boundary is the publish: the arena, ent[] and live words a
 * probe kernel reads were all written by an earlier kernel.  A stale zero
 * read of a slot word is harmless (the CAS then returns the real word) and
 * a non-zero word never changes while a probe kernel runs.  Every loop is
 * bounded by the table capacity or the string length and ends in an error
 * code.
 */
#include <hipcub/hipcub.hpp>

#include <climits>

#include "op_common.h"

namespace strkey {

#define SK_PENDING 0x80000000ull
#define SK_LIVE 1ull
#define SK_DEAD 2ull

#define SKERR_OFFSETS 1
#define SKERR_CAPACITY 2
#define SKERR_ARENA 3
#define SKERR_BAD_ID 4
#define SKERR_RESTORE 5

#define SK_ALIGN 8 /* arena padding per string: at most SK_ALIGN - 1 bytes */

struct Ent {
    int64_t off;
    int64_t len;
};

/* device counters; the first 8 bytes are re-zeroed before every call */
struct Ctr {
    int err;
    unsigned n_win;
    unsigned long long arena_used;
    unsigned long long n_live;
    unsigned long long occupied; /* live + dead */
};

struct Table {
    unsigned long long *slots;
    Ent *ent;
    uint8_t *arena;
    int64_t arena_bytes;
    uint64_t mask;      /* cap - 1 */
    uint64_t hash_mask; /* ~0 or (1 << hash_bits) - 1 */
    Ctr *ctr;
};

__device__ inline uint64_t load8(const uint8_t *p) {
    uint64_t w;
    __builtin_memcpy(&w, p, 8);
    return w;
}

__device__ inline uint64_t rotl64(uint64_t x, int r) {
    return (x << r) | (x >> (64 - r));
}

__device__ inline uint64_t hash_step(uint64_t h, uint64_t w) {
    w *= 0x87c37b91114253d5ull;
    w = rotl64(w, 31);
    w *= 0x4cf5ad432745937full;
    h ^= w;
    h = rotl64(h, 27);
    return h * 5 + 0x52dce729ull;
}

/* 64-bit content hash (MurmurHash3-style block mix and finaliser): a pure
 * function of the bytes and the length, whatever their alignment.  Reads
 * exactly p[0 .. n). */
__device__ inline uint64_t content_hash(const uint8_t *p, int64_t n) {
    uint64_t h = 0x9e3779b97f4a7c15ull ^ ((uint64_t)n * 0xff51afd7ed558ccdull);
    int64_t i = 0;
    for (; i + 8 <= n; i += 8) h = hash_step(h, load8(p + i));
    if (i < n) {
        uint64_t w = 0;
        for (int j = 0; i + j < n; j++) w |= (uint64_t)p[i + j] << (8 * j);
        h = hash_step(h, w);
    }
    h ^= (uint64_t)n;
    h ^= h >> 33;
    h *= 0xff51afd7ed558ccdull;
    h ^= h >> 33;
    h *= 0xc4ceb9fe1a85ec53ull;
    h ^= h >> 33;
    return h;
}

/* exact compare of a[0 .. n) and b[0 .. n); reads nothing outside them */
__device__ inline bool bytes_eq(const uint8_t *a, const uint8_t *b, int64_t n) {
    int64_t i = 0;
    for (; i + 8 <= n; i += 8)
        if (load8(a + i) != load8(b + i)) return false;
    for (; i < n; i++)
        if (a[i] != b[i]) return false;
    return true;
}

__device__ inline void copy_bytes(uint8_t *dst, const uint8_t *src, int64_t n) {
    int64_t i = 0;
    for (; i + 8 <= n; i += 8) {
        uint64_t w = load8(src + i);
        __builtin_memcpy(dst + i, &w, 8);
    }
    for (; i < n; i++) dst[i] = src[i];
}

/* Arrow offsets must be non-negative and non-decreasing.  Runs to
 * completion before any kernel dereferences `data`. */
__global__ void __launch_bounds__(256)
k_strkey_check_offsets(const int32_t *off, int64_t n_rows, Ctr *ctr) {
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         r < n_rows; r += stride)
        if (off[r] < 0 || off[r + 1] < off[r])
            atomicMax(&ctr->err, SKERR_OFFSETS);
}

/* `data` is addressed as data[off - bias]: the host surface stages only
 * bytes [offsets[0], offsets[n_rows]) and passes bias = offsets[0]. */
__global__ void __launch_bounds__(256)
k_strkey_probe(Table T, const int32_t *off, const uint8_t *data, int64_t bias,
               int64_t n_rows, int64_t *ids, uint64_t *hashes,
               unsigned *win_rows) {
    if (T.ctr->err) return; /* malformed offsets: touch no byte */
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         r < n_rows; r += stride) {
        const uint8_t *p = data + ((int64_t)off[r] - bias);
        const int64_t len = (int64_t)off[r + 1] - off[r];
        const uint64_t full = content_hash(p, len);
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
                    (tag << 32) | SK_PENDING | (unsigned long long)(r + 1);
                w = atomicCAS(&T.slots[slot], 0ull, mine);
                if (w == 0) {
                    win_rows[atomicAdd(&T.ctr->n_win, 1u)] = (unsigned)r;
                    id = (int64_t)slot;
                    break;
                }
            }
            if ((w >> 32) != tag) continue;
            if (w & SK_PENDING) {
                const int64_t j = (int64_t)(w & 0x7fffffffull) - 1;
                if ((int64_t)off[j + 1] - off[j] == len &&
                    bytes_eq(p, data + ((int64_t)off[j] - bias), len)) {
                    id = (int64_t)slot;
                    break;
                }
            } else if ((w & 0xffffffffull) == SK_LIVE) {
                const Ent e = T.ent[slot];
                if (e.len == len && bytes_eq(p, T.arena + e.off, len)) {
                    id = (int64_t)slot;
                    break;
                }
            }
        }
        if (id < 0) atomicMax(&T.ctr->err, SKERR_CAPACITY);
        ids[r] = id;
    }
}

/* Winners only.  occ0 = occupied slots before this call, max_occ = the
 * load limit; a winner past either limit turns its slot DEAD. */
__global__ void __launch_bounds__(256)
k_strkey_publish(Table T, const int32_t *off, const uint8_t *data,
                 int64_t bias, const int64_t *ids, const unsigned *win_rows,
                 uint64_t occ0, uint64_t max_occ) {
    const unsigned n_win = T.ctr->n_win;
    unsigned stride = gridDim.x * blockDim.x;
    for (unsigned w = blockIdx.x * blockDim.x + threadIdx.x; w < n_win;
         w += stride) {
        const int64_t r = win_rows[w];
        const int64_t slot = ids[r];
        const int64_t len = (int64_t)off[r + 1] - off[r];
        const int64_t pad = (len + SK_ALIGN - 1) & ~(int64_t)(SK_ALIGN - 1);
        const unsigned long long tagw =
            T.slots[slot] & 0xffffffff00000000ull;
        atomicAdd(&T.ctr->occupied, 1ull);
        if (occ0 + w >= max_occ) {
            T.slots[slot] = tagw | SK_DEAD;
            atomicMax(&T.ctr->err, SKERR_CAPACITY);
            continue;
        }
        const unsigned long long a =
            atomicAdd(&T.ctr->arena_used, (unsigned long long)pad);
        if (a + (unsigned long long)pad > (unsigned long long)T.arena_bytes) {
            atomicAdd(&T.ctr->arena_used, (unsigned long long)(-pad));
            T.slots[slot] = tagw | SK_DEAD;
            atomicMax(&T.ctr->err, SKERR_ARENA);
            continue;
        }
        copy_bytes(T.arena + a, data + ((int64_t)off[r] - bias), len);
        Ent e = {(int64_t)a, len};
        T.ent[slot] = e;
        T.slots[slot] = tagw | SK_LIVE;
        atomicAdd(&T.ctr->n_live, 1ull);
    }
}

/* decode step 1: lengths of the requested ids (never-issued id = error) */
__global__ void __launch_bounds__(256)
k_strkey_dec_len(Table T, const int64_t *ids, int64_t n, int64_t *lens) {
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += stride) {
        const int64_t id = ids[i];
        int64_t len = 0;
        if (id < 0 || (uint64_t)id > T.mask ||
            (T.slots[id] & 0xffffffffull) != SK_LIVE)
            atomicMax(&T.ctr->err, SKERR_BAD_ID);
        else
            len = T.ent[id].len;
        lens[i] = len;
    }
}

/* decode step 3: gather bytes; pos = exclusive scan of lens.  Runs only
 * after the host saw err == 0 and a total <= INT32_MAX. */
__global__ void __launch_bounds__(256)
k_strkey_dec_gather(Table T, const int64_t *ids, const int64_t *pos,
                    const int64_t *lens, int64_t n, int32_t *out_off,
                    uint8_t *out_data) {
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += stride) {
        out_off[i] = (int32_t)pos[i];
        if (i == n - 1) out_off[n] = (int32_t)(pos[i] + lens[i]);
        copy_bytes(out_data + pos[i], T.arena + T.ent[ids[i]].off, lens[i]);
    }
}

/* drain: flag live slots, scan, compact their ids in slot order */
__global__ void __launch_bounds__(256)
k_strkey_live_flags(Table T, int64_t *flags) {
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         s <= (int64_t)T.mask; s += stride)
        flags[s] = (T.slots[s] & 0xffffffffull) == SK_LIVE;
}

__global__ void __launch_bounds__(256)
k_strkey_live_ids(Table T, const int64_t *flags, const int64_t *pos,
                  int64_t *ids) {
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         s <= (int64_t)T.mask; s += stride)
        if (flags[s]) ids[pos[s]] = s;
}

/* restore step 1: place every string at the slot its id names */
__global__ void __launch_bounds__(256)
k_strkey_restore_place(Table T, const int64_t *ids, const int32_t *off,
                       const uint8_t *data, int64_t bias, int64_t n_rows) {
    if (T.ctr->err) return;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         r < n_rows; r += stride) {
        const int64_t id = ids[r];
        if (id < 0 || (uint64_t)id > T.mask) {
            atomicMax(&T.ctr->err, SKERR_RESTORE);
            continue;
        }
        const uint8_t *p = data + ((int64_t)off[r] - bias);
        const int64_t len = (int64_t)off[r + 1] - off[r];
        const uint64_t h = content_hash(p, len) & T.hash_mask;
        const unsigned long long word = ((h >> 32) << 32) | SK_LIVE;
        if (atomicCAS(&T.slots[id], 0ull, word) != 0) { /* duplicate id */
            atomicMax(&T.ctr->err, SKERR_RESTORE);
            continue;
        }
        const int64_t pad = (len + SK_ALIGN - 1) & ~(int64_t)(SK_ALIGN - 1);
        const unsigned long long a =
            atomicAdd(&T.ctr->arena_used, (unsigned long long)pad);
        if (a + (unsigned long long)pad > (unsigned long long)T.arena_bytes) {
            atomicMax(&T.ctr->err, SKERR_ARENA);
            Ent none = {0, 0};
            T.ent[id] = none;
            continue;
        }
        copy_bytes(T.arena + a, p, len);
        Ent e = {(int64_t)a, len};
        T.ent[id] = e;
        atomicAdd(&T.ctr->n_live, 1ull);
        atomicAdd(&T.ctr->occupied, 1ull);
    }
}

/* restore step 2 (next kernel, so the whole table is visible): a later
 * lookup of row r must reach slot ids[r] -- no empty slot and no equal
 * string on the probe path from its home slot. */
__global__ void __launch_bounds__(256)
k_strkey_restore_verify(Table T, const int64_t *ids, const int32_t *off,
                        const uint8_t *data, int64_t bias, int64_t n_rows) {
    if (T.ctr->err) return;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         r < n_rows; r += stride) {
        const uint8_t *p = data + ((int64_t)off[r] - bias);
        const int64_t len = (int64_t)off[r + 1] - off[r];
        const uint64_t h = content_hash(p, len) & T.hash_mask;
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
            if ((w >> 32) == tag) {
                const Ent e = T.ent[slot];
                if (e.len == len && bytes_eq(p, T.arena + e.off, len)) break;
            }
        }
        if (!ok) atomicMax(&T.ctr->err, SKERR_RESTORE);
    }
}

}  // namespace strkey

using namespace strkey;

struct GpuStrKey : OpBase {
    AmdStrKeyConfig cfg;
    Table T;
    uint64_t cap, max_occ;
    /* host mirrors of the device counters, refreshed after every call */
    uint64_t n_live, occupied, arena_used;
    /* per-batch scratch, grown on demand */
    unsigned *d_win;
    int64_t win_cap;
    int32_t *d_off;
    int64_t off_cap;
    uint8_t *d_data;
    int64_t data_cap;
    int64_t *d_ids;
    int64_t ids_cap;
    uint64_t *d_hashes;
    int64_t hashes_cap;
    /* opt-in timing of the probe kernel (arroyo_amd_strkey_profile) */
    int prof_on;
    hipEvent_t ev0, ev1;
    double last_probe_ms;
};

template <typename P>
static int sk_grow(GpuStrKey *o, P **buf, int64_t *cap, int64_t want,
                   size_t elem) {
    if (want <= *cap) return 0;
    /* allocations belong on the handle's device, whatever the caller's
     * current one is */
    HIP_CHECK(o, hipSetDevice(o->cfg.device));
    int64_t n = *cap ? *cap : 1024;
    while (n < want) n *= 2;
    o->release(*buf);
    *cap = 0;
    HIP_CHECK(o, o->dev_alloc(*buf, (size_t)n * elem));
    *cap = n;
    return 0;
}

API void *arroyo_amd_strkey_create(const AmdStrKeyConfig *cfg) {
    if (!cfg || cfg->log2_capacity < 1 || cfg->log2_capacity > 30 ||
        cfg->arena_bytes < 1 || cfg->hash_bits < 0 || cfg->hash_bits > 63) {
        snprintf(g_create_err, sizeof g_create_err,
                 "invalid strkey config (log2_capacity 1..30, arena_bytes "
                 ">= 1, hash_bits 0..63)");
        return nullptr;
    }
    if (hipSetDevice(cfg->device) != hipSuccess) {
        snprintf(g_create_err, sizeof g_create_err,
                 "hipSetDevice(%d) failed: no HIP device (no CPU fallback)",
                 cfg->device);
        return nullptr;
    }
    GpuStrKey *o = new GpuStrKey();
    o->cfg = *cfg;
    o->cap = 1ull << cfg->log2_capacity;
    /* load limit 7/8: keeps a free slot on every probe path */
    o->max_occ = o->cap - o->cap / 8;
    o->T.mask = o->cap - 1;
    o->T.hash_mask = cfg->hash_bits ? (1ull << cfg->hash_bits) - 1 : ~0ull;
    o->T.arena_bytes = cfg->arena_bytes;
    OP_TRY(o, "strkey alloc", o->dev_alloc(o->T.slots, o->cap * 8, 0));
    OP_TRY(o, "strkey alloc", o->dev_alloc(o->T.ent, o->cap * sizeof(Ent)));
    OP_TRY(o, "strkey alloc",
           o->dev_alloc(o->T.arena, (size_t)cfg->arena_bytes));
    OP_TRY(o, "strkey alloc", o->dev_alloc(o->T.ctr, sizeof(Ctr), 0));
    OP_TRY(o, "strkey alloc", o->stream_create(&o->stream));
    return o;
}

API const char *arroyo_amd_strkey_last_error(void *h) {
    return h ? ((GpuStrKey *)h)->err_msg : g_create_err;
}

/* read the counters back (synchronises the stream) and refresh the mirrors */
static int sk_sync_counters(GpuStrKey *o, Ctr *c) {
    HIP_CHECK(o, hipMemcpyAsync(c, o->T.ctr, sizeof(Ctr), hipMemcpyDeviceToHost,
                               o->stream));
    HIP_CHECK(o, hipStreamSynchronize(o->stream));
    o->n_live = c->n_live;
    o->occupied = c->occupied;
    o->arena_used = c->arena_used;
    return 0;
}

static int sk_report(GpuStrKey *o, int err) {
    switch (err) {
    case 0:
        return 0;
    case SKERR_OFFSETS:
        snprintf(o->err_msg, sizeof o->err_msg,
                 "malformed offsets: negative or decreasing");
        break;
    case SKERR_CAPACITY:
        snprintf(o->err_msg, sizeof o->err_msg,
                 "dictionary capacity exhausted: %llu of %llu slots in use "
                 "(limit %llu); raise log2_capacity",
                 (unsigned long long)o->occupied, (unsigned long long)o->cap,
                 (unsigned long long)o->max_occ);
        break;
    case SKERR_ARENA:
        snprintf(o->err_msg, sizeof o->err_msg,
                 "string arena full: %llu of %lld bytes in use; raise "
                 "arena_bytes",
                 (unsigned long long)o->arena_used,
                 (long long)o->cfg.arena_bytes);
        break;
    case SKERR_BAD_ID:
        snprintf(o->err_msg, sizeof o->err_msg,
                 "decode of an id this dictionary never issued");
        break;
    default:
        snprintf(o->err_msg, sizeof o->err_msg,
                 "restore: an id is out of range, duplicated or not "
                 "reachable from its string's home slot (log2_capacity and "
                 "hash_bits must match the drained handle)");
    }
    return 1;
}

/* the encode core: offsets, data and outputs all on the device */
static int sk_encode_device(GpuStrKey *o, const int32_t *d_off,
                            const uint8_t *d_data, int64_t bias,
                            int64_t n_rows, int64_t *d_ids,
                            uint64_t *d_hashes) {
    if (n_rows < 0 || n_rows > INT32_MAX - 1) {
        snprintf(o->err_msg, sizeof o->err_msg, "invalid n_rows %lld",
                 (long long)n_rows);
        return 1;
    }
    if (n_rows == 0) return 0;
    if (sk_grow(o, &o->d_win, &o->win_cap, n_rows, sizeof(unsigned))) return 1;
    HIP_CHECK(o, hipMemsetAsync(o->T.ctr, 0, 8, o->stream));
    const int grid = grid_for(n_rows, 2048);
    hipLaunchKernelGGL(k_strkey_check_offsets, dim3(grid), dim3(256), 0,
                       o->stream, d_off, n_rows, o->T.ctr);
    if (o->prof_on) HIP_CHECK(o, hipEventRecord(o->ev0, o->stream));
    hipLaunchKernelGGL(k_strkey_probe, dim3(grid), dim3(256), 0, o->stream,
                       o->T, d_off, d_data, bias, n_rows, d_ids, d_hashes,
                       o->d_win);
    if (o->prof_on) HIP_CHECK(o, hipEventRecord(o->ev1, o->stream));
    hipLaunchKernelGGL(k_strkey_publish, dim3(256), dim3(256), 0, o->stream,
                       o->T, d_off, d_data, bias, (const int64_t *)d_ids,
                       (const unsigned *)o->d_win, o->occupied, o->max_occ);
    HIP_CHECK(o, hipGetLastError());
    Ctr c;
    if (sk_sync_counters(o, &c)) return 1;
    if (o->prof_on) {
        float ms = 0.f;
        HIP_CHECK(o, hipEventElapsedTime(&ms, o->ev0, o->ev1));
        o->last_probe_ms = ms;
    }
    return sk_report(o, c.err);
}

API int arroyo_amd_strkey_profile(void *h, int enable,
                                  double *last_lookup_ms) {
    GpuStrKey *o = (GpuStrKey *)h;
    if (enable > 0 && !o->ev0) {
        HIP_CHECK(o, hipSetDevice(o->cfg.device));
        HIP_CHECK(o, o->event_create(&o->ev0));
        HIP_CHECK(o, o->event_create(&o->ev1));
    }
    if (enable >= 0) o->prof_on = enable > 0;
    if (last_lookup_ms) *last_lookup_ms = o->last_probe_ms;
    return 0;
}

API int arroyo_amd_strkey_encode_device(void *h, const int32_t *d_offsets,
                                        const uint8_t *d_data, int64_t n_rows,
                                        int64_t *d_ids_out,
                                        uint64_t *d_hashes_out) {
    return sk_encode_device((GpuStrKey *)h, d_offsets, d_data, 0, n_rows,
                            d_ids_out, d_hashes_out);
}

/* stage offsets[0 .. n_rows] and data[offsets[0] .. offsets[n_rows]) */
static int sk_stage(GpuStrKey *o, const int32_t *offsets, const uint8_t *data,
                    int64_t n_rows, int64_t *bias) {
    const int64_t lo = offsets[0], hi = offsets[n_rows];
    if (lo < 0 || hi < lo) {
        snprintf(o->err_msg, sizeof o->err_msg,
                 "malformed offsets: negative or decreasing");
        return 1;
    }
    if (sk_grow(o, &o->d_off, &o->off_cap, n_rows + 1, 4)) return 1;
    if (sk_grow(o, &o->d_data, &o->data_cap, hi - lo + 1, 1)) return 1;
    HIP_CHECK(o, hipMemcpyAsync(o->d_off, offsets, (size_t)(n_rows + 1) * 4,
                               hipMemcpyHostToDevice, o->stream));
    if (hi > lo)
        HIP_CHECK(o, hipMemcpyAsync(o->d_data, data + lo, (size_t)(hi - lo),
                                   hipMemcpyHostToDevice, o->stream));
    *bias = lo;
    return 0;
}

API int arroyo_amd_strkey_encode(void *h, const int32_t *offsets,
                                 const uint8_t *data, int64_t n_rows,
                                 int64_t *ids_out, uint64_t *hashes_out) {
    GpuStrKey *o = (GpuStrKey *)h;
    if (n_rows == 0) return 0;
    if (n_rows < 0 || n_rows > INT32_MAX - 1) {
        snprintf(o->err_msg, sizeof o->err_msg, "invalid n_rows %lld",
                 (long long)n_rows);
        return 1;
    }
    int64_t bias = 0;
    if (sk_stage(o, offsets, data, n_rows, &bias)) return 1;
    if (sk_grow(o, &o->d_ids, &o->ids_cap, n_rows, 8)) return 1;
    if (hashes_out &&
        sk_grow(o, &o->d_hashes, &o->hashes_cap, n_rows, 8))
        return 1;
    if (sk_encode_device(o, o->d_off, o->d_data, bias, n_rows, o->d_ids,
                         hashes_out ? o->d_hashes : nullptr))
        return 1;
    HIP_CHECK(o, hipMemcpyAsync(ids_out, o->d_ids, (size_t)n_rows * 8,
                               hipMemcpyDeviceToHost, o->stream));
    if (hashes_out)
        HIP_CHECK(o, hipMemcpyAsync(hashes_out, o->d_hashes, (size_t)n_rows * 8,
                                   hipMemcpyDeviceToHost, o->stream));
    HIP_CHECK(o, hipStreamSynchronize(o->stream));
    return 0;
}

API void arroyo_amd_strkey_free_out(AmdStrBatch *out);

/* a host allocation of an output batch failed: free the batch, say so */
static int sk_out_oom(GpuStrKey *o, AmdStrBatch *out) {
    arroyo_amd_strkey_free_out(out);
    snprintf(o->err_msg, sizeof o->err_msg,
             "strkey output: host allocation failed");
    return 1;
}

static int sk_empty_out(GpuStrKey *o, AmdStrBatch *out) {
    out->n_rows = 0;
    out->ids = (int64_t *)malloc(8);
    out->offsets = (int32_t *)malloc(4);
    out->data = (uint8_t *)malloc(1);
    if (!out->ids || !out->offsets || !out->data) return sk_out_oom(o, out);
    out->offsets[0] = 0;
    return 0;
}

struct DecTmp {
    int64_t *lens = nullptr, *pos = nullptr;
    void *cub = nullptr;
    int32_t *off = nullptr;
    uint8_t *data = nullptr;
    ~DecTmp() {
        (void)hipFree(lens);
        (void)hipFree(pos);
        (void)hipFree(cub);
        (void)hipFree(off);
        (void)hipFree(data);
    }
};

/* decode n device-resident ids into malloc'd host buffers: gather lengths,
 * hipCUB exclusive scan, gather bytes, copy out.  out->ids is left alone. */
static int sk_decode_device_ids(GpuStrKey *o, const int64_t *d_ids, int64_t n,
                                AmdStrBatch *out) {
    DecTmp t;
    HIP_CHECK(o, hipSetDevice(o->cfg.device));
    HIP_CHECK(o, hipMalloc((void **)&t.lens, (size_t)n * 8));
    HIP_CHECK(o, hipMalloc((void **)&t.pos, (size_t)n * 8));
    HIP_CHECK(o, hipMalloc((void **)&t.off, (size_t)(n + 1) * 4));
    size_t cub_bytes = 0;
    HIP_CHECK(o, hipcub::DeviceScan::ExclusiveSum(nullptr, cub_bytes, t.lens,
                                                 t.pos, (int)n));
    HIP_CHECK(o, hipMalloc(&t.cub, cub_bytes ? cub_bytes : 1));
    HIP_CHECK(o, hipMemsetAsync(o->T.ctr, 0, 8, o->stream));
    const int grid = grid_for(n, 2048);
    hipLaunchKernelGGL(k_strkey_dec_len, dim3(grid), dim3(256), 0, o->stream,
                       o->T, d_ids, n, t.lens);
    HIP_CHECK(o, hipGetLastError());
    HIP_CHECK(o, hipcub::DeviceScan::ExclusiveSum(t.cub, cub_bytes, t.lens,
                                                  t.pos, (int)n, o->stream));
    int64_t tail[2] = {0, 0};
    HIP_CHECK(o, hipMemcpyAsync(&tail[0], t.pos + (n - 1), 8,
                               hipMemcpyDeviceToHost, o->stream));
    HIP_CHECK(o, hipMemcpyAsync(&tail[1], t.lens + (n - 1), 8,
                               hipMemcpyDeviceToHost, o->stream));
    Ctr c;
    if (sk_sync_counters(o, &c)) return 1;
    if (c.err) return sk_report(o, c.err);
    const int64_t total = tail[0] + tail[1];
    if (total > INT32_MAX) {
        snprintf(o->err_msg, sizeof o->err_msg,
                 "decoded strings total %lld bytes, above the int32 offset "
                 "range of a Utf8 array",
                 (long long)total);
        return 1;
    }
    HIP_CHECK(o, hipMalloc((void **)&t.data, total ? (size_t)total : 1));
    hipLaunchKernelGGL(k_strkey_dec_gather, dim3(grid), dim3(256), 0,
                       o->stream, o->T, d_ids, (const int64_t *)t.pos,
                       (const int64_t *)t.lens, n, t.off, t.data);
    HIP_CHECK(o, hipGetLastError());
    out->offsets = (int32_t *)malloc((size_t)(n + 1) * 4);
    out->data = (uint8_t *)malloc(total ? (size_t)total : 1);
    if (!out->offsets || !out->data) return sk_out_oom(o, out);
    HIP_CHECK(o, hipMemcpyAsync(out->offsets, t.off, (size_t)(n + 1) * 4,
                               hipMemcpyDeviceToHost, o->stream));
    if (total)
        HIP_CHECK(o, hipMemcpyAsync(out->data, t.data, (size_t)total,
                                   hipMemcpyDeviceToHost, o->stream));
    HIP_CHECK(o, hipStreamSynchronize(o->stream));
    return 0;
}

API void arroyo_amd_strkey_free_out(AmdStrBatch *out) {
    if (!out) return;
    free(out->ids);
    free(out->offsets);
    free(out->data);
    memset(out, 0, sizeof *out);
}

API int arroyo_amd_strkey_decode(void *h, const int64_t *ids, int64_t n_rows,
                                 AmdStrBatch *out) {
    GpuStrKey *o = (GpuStrKey *)h;
    memset(out, 0, sizeof *out);
    if (n_rows < 0 || n_rows > INT32_MAX - 1) {
        snprintf(o->err_msg, sizeof o->err_msg, "invalid n_rows %lld",
                 (long long)n_rows);
        return 1;
    }
    if (n_rows == 0) return sk_empty_out(o, out);
    if (sk_grow(o, &o->d_ids, &o->ids_cap, n_rows, 8)) return 1;
    HIP_CHECK(o, hipMemcpyAsync(o->d_ids, ids, (size_t)n_rows * 8,
                               hipMemcpyHostToDevice, o->stream));
    int rc = sk_decode_device_ids(o, o->d_ids, n_rows, out);
    if (rc) {
        arroyo_amd_strkey_free_out(out);
        return rc;
    }
    out->n_rows = n_rows;
    out->ids = (int64_t *)malloc((size_t)n_rows * 8);
    if (!out->ids) return sk_out_oom(o, out);
    memcpy(out->ids, ids, (size_t)n_rows * 8);
    return 0;
}

API int arroyo_amd_strkey_count(void *h, int64_t *n_strings,
                                int64_t *arena_used) {
    GpuStrKey *o = (GpuStrKey *)h;
    if (n_strings) *n_strings = (int64_t)o->n_live;
    if (arena_used) *arena_used = (int64_t)o->arena_used;
    return 0;
}

struct DrainTmp {
    int64_t *flags = nullptr, *pos = nullptr, *ids = nullptr;
    void *cub = nullptr;
    ~DrainTmp() {
        (void)hipFree(flags);
        (void)hipFree(pos);
        (void)hipFree(ids);
        (void)hipFree(cub);
    }
};

API int arroyo_amd_strkey_checkpoint_drain(void *h, AmdStrBatch *out) {
    GpuStrKey *o = (GpuStrKey *)h;
    memset(out, 0, sizeof *out);
    const int64_t n = (int64_t)o->n_live;
    if (n == 0) return sk_empty_out(o, out);
    DrainTmp t;
    const int64_t cap = (int64_t)o->cap;
    HIP_CHECK(o, hipSetDevice(o->cfg.device));
    HIP_CHECK(o, hipMalloc((void **)&t.flags, (size_t)cap * 8));
    HIP_CHECK(o, hipMalloc((void **)&t.pos, (size_t)cap * 8));
    HIP_CHECK(o, hipMalloc((void **)&t.ids, (size_t)n * 8));
    size_t cub_bytes = 0;
    HIP_CHECK(o, hipcub::DeviceScan::ExclusiveSum(nullptr, cub_bytes, t.flags,
                                                 t.pos, (int)cap));
    HIP_CHECK(o, hipMalloc(&t.cub, cub_bytes ? cub_bytes : 1));
    const int grid = grid_for(cap, 2048);
    hipLaunchKernelGGL(k_strkey_live_flags, dim3(grid), dim3(256), 0,
                       o->stream, o->T, t.flags);
    HIP_CHECK(o, hipcub::DeviceScan::ExclusiveSum(t.cub, cub_bytes, t.flags,
                                                  t.pos, (int)cap,
                                                  o->stream));
    hipLaunchKernelGGL(k_strkey_live_ids, dim3(grid), dim3(256), 0, o->stream,
                       o->T, (const int64_t *)t.flags, (const int64_t *)t.pos,
                       t.ids);
    HIP_CHECK(o, hipGetLastError());
    int rc = sk_decode_device_ids(o, t.ids, n, out);
    if (rc) {
        arroyo_amd_strkey_free_out(out);
        return rc;
    }
    out->n_rows = n;
    out->ids = (int64_t *)malloc((size_t)n * 8);
    if (!out->ids) return sk_out_oom(o, out);
    hipError_t e =
        hipMemcpy(out->ids, t.ids, (size_t)n * 8, hipMemcpyDeviceToHost);
    if (e != hipSuccess) {
        arroyo_amd_strkey_free_out(out);
        HIP_CHECK(o, e);
    }
    return 0;
}

API int arroyo_amd_strkey_restore(void *h, const int64_t *ids,
                                  const int32_t *offsets, const uint8_t *data,
                                  int64_t n_rows) {
    GpuStrKey *o = (GpuStrKey *)h;
    if (o->occupied != 0) {
        snprintf(o->err_msg, sizeof o->err_msg,
                 "restore into a non-empty dictionary (%llu strings held)",
                 (unsigned long long)o->n_live);
        return 1;
    }
    if (n_rows == 0) return 0;
    if (n_rows < 0 || (uint64_t)n_rows > o->max_occ) {
        snprintf(o->err_msg, sizeof o->err_msg,
                 "restore of %lld strings exceeds the dictionary capacity "
                 "(limit %llu of %llu slots)",
                 (long long)n_rows, (unsigned long long)o->max_occ,
                 (unsigned long long)o->cap);
        return 1;
    }
    int64_t bias = 0;
    if (sk_stage(o, offsets, data, n_rows, &bias)) return 1;
    if (sk_grow(o, &o->d_ids, &o->ids_cap, n_rows, 8)) return 1;
    HIP_CHECK(o, hipMemcpyAsync(o->d_ids, ids, (size_t)n_rows * 8,
                               hipMemcpyHostToDevice, o->stream));
    HIP_CHECK(o, hipMemsetAsync(o->T.ctr, 0, 8, o->stream));
    const int grid = grid_for(n_rows, 2048);
    hipLaunchKernelGGL(k_strkey_check_offsets, dim3(grid), dim3(256), 0,
                       o->stream, (const int32_t *)o->d_off, n_rows, o->T.ctr);
    hipLaunchKernelGGL(k_strkey_restore_place, dim3(grid), dim3(256), 0,
                       o->stream, o->T, (const int64_t *)o->d_ids,
                       (const int32_t *)o->d_off, (const uint8_t *)o->d_data,
                       bias, n_rows);
    hipLaunchKernelGGL(k_strkey_restore_verify, dim3(grid), dim3(256), 0,
                       o->stream, o->T, (const int64_t *)o->d_ids,
                       (const int32_t *)o->d_off, (const uint8_t *)o->d_data,
                       bias, n_rows);
    HIP_CHECK(o, hipGetLastError());
    Ctr c;
    if (sk_sync_counters(o, &c)) return 1;
    if (c.err) {
        /* a failed restore leaves the handle empty, not half loaded */
        int rc = sk_report(o, c.err);
        HIP_CHECK(o, hipMemsetAsync(o->T.slots, 0, o->cap * 8, o->stream));
        HIP_CHECK(o, hipMemsetAsync(o->T.ctr, 0, sizeof(Ctr), o->stream));
        HIP_CHECK(o, hipStreamSynchronize(o->stream));
        o->n_live = o->occupied = o->arena_used = 0;
        return rc;
    }
    return 0;
}

API void arroyo_amd_strkey_destroy(void *h) {
    delete (GpuStrKey *)h;   /* ~OpBase drains the stream first */
}
