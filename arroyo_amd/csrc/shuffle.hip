/* arroyo-amd keyed shuffle, device side: MI355X-native (gfx950) stable
 * N-column partition with an optional Arrow Utf8 column, behind the
 * arroyo_amd_shuffle_* C ABI (include/arroyo_amd.h).
 *
 * The reference's cross-subtask repartition (crates/arroyo-operator/src/
 * context.rs:506-560) sorts a batch by destination and slices it, so every
 * destination receives its rows in input order.  This family does the same
 * on device: partition p occupies rows [row_start[p], row_start[p + 1]) of
 * every output column, in input order (a stable counting sort by owner).
 *
 * Five kernels on the handle's own stream; the kernel boundary is the only
 * synchronisation between blocks and no block ever waits on another.  Every
 * block of the count and scatter kernels owns the same fixed tile of
 * SHUF_TILE consecutive rows.
 *   k_shuf_count         owner of every row -> uint8 plane; per-block
 *                        histogram (and byte sums) in LDS -> hist[p][block].
 *                        Validates the Utf8 offsets; touches no string byte.
 *   k_shuf_scan          one block: exclusive scan of hist in partition-major,
 *                        block-minor order -> each block's base per partition,
 *                        row_start[], byte_start[]; flags bytes > max_bytes.
 *   k_shuf_scatter       the tile again: a row's rank among the lanes of its
 *                        wave with the same owner is a ballot and a popcount
 *                        of the lower lanes; per-(pass, wave, owner) counts
 *                        are prefixed through LDS.  All columns move in this
 *                        pass; a string's length and source offset go to its
 *                        destination slot.
 *   k_shuf_utf8_offsets  one wave per (partition, source block) run of
 *                        destination rows: wave prefix sums of the lengths on
 *                        top of the run's byte base from k_shuf_scan, rebased
 *                        per partition.
 *   k_shuf_utf8_copy     one wave per 64 destination rows: a lane copies its
 *                        own string when it is short, the whole wave copies
 *                        the long ones together.
 * The two Utf8 kernels return at once when the error word is set, so a
 * malformed offsets array never leads to a dereference of `data`.
 */
#include <hipcub/hipcub.hpp>

#include <climits>

#include "op_common.h"

namespace shuf {

#define SHUF_BLOCK 256
#define SHUF_WAVES (SHUF_BLOCK / 64)
#define SHUF_PASSES 4
#define SHUF_TILE (SHUF_BLOCK * SHUF_PASSES) /* rows per block */
static_assert(SHUF_TILE == AMD_SHUF_TILE_ROWS, "tile size is part of the header");
#define SHUF_SCAN_THREADS 1024
/* strings up to this many bytes are copied by their own lane */
#define SHUF_COPY_THRESHOLD 32

/* raised with atomicMax: malformed offsets outrank the byte limit, whose
 * sum means nothing then */
#define SHERR_BYTES 1
#define SHERR_OFFSETS 2

/* what the scan kernel leaves for the host: 8-byte fields only */
struct Starts {
    int64_t row[AMD_SHUF_MAX_PARTS + 1];
    int64_t byte[AMD_SHUF_MAX_PARTS + 1];
    int64_t err;
};

struct ColPtrs {
    const int64_t *in[AMD_SHUF_MAX_COLS];
    int64_t *out[AMD_SHUF_MAX_COLS];
};

/* range == 0 stands for n_parts == 1 */
__device__ inline uint32_t owner_of(int64_t key, int key_mode, uint64_t range) {
    if (range == 0) return 0;
    /* hash64: the splitmix64 finaliser of arroyo_amd_partition */
    const uint64_t h =
        key_mode == AMD_SHUF_KEY_HASH ? (uint64_t)key : hash64((uint64_t)key);
    return (uint32_t)(h / range);
}

__global__ void __launch_bounds__(SHUF_BLOCK)
k_shuf_count(const int64_t *keys, const int32_t *off, int64_t n_rows,
             int n_parts, int key_mode, uint8_t *owner, uint32_t *hist_rows,
             uint32_t *hist_bytes, int n_blocks, int *err) {
    __shared__ uint32_t cnt[AMD_SHUF_MAX_PARTS];
    __shared__ uint32_t bytes[AMD_SHUF_MAX_PARTS];
    const int tid = threadIdx.x;
    if (tid < AMD_SHUF_MAX_PARTS) {
        cnt[tid] = 0;
        bytes[tid] = 0;
    }
    __syncthreads();
    const uint64_t range = n_parts > 1 ? (~0ULL / (uint64_t)n_parts) + 1 : 0;
    const int64_t base = (int64_t)blockIdx.x * SHUF_TILE;
    for (int it = 0; it < SHUF_PASSES; it++) {
        const int64_t r = base + it * SHUF_BLOCK + tid;
        if (r >= n_rows) break;
        const uint32_t o = owner_of(keys[r], key_mode, range);
        owner[r] = (uint8_t)o;
        atomicAdd(&cnt[o], 1u);
        if (off) {
            const int32_t a = off[r], b = off[r + 1];
            if (a < 0 || b < a)
                atomicMax(err, SHERR_OFFSETS);
            else
                atomicAdd(&bytes[o], (uint32_t)(b - a));
        }
    }
    __syncthreads();
    if (tid < n_parts) {
        hist_rows[(int64_t)tid * n_blocks + blockIdx.x] = cnt[tid];
        if (off) hist_bytes[(int64_t)tid * n_blocks + blockIdx.x] = bytes[tid];
    }
}

typedef hipcub::BlockScan<uint32_t, SHUF_SCAN_THREADS> ScanT;

/* exclusive scan of in[0 .. n) by one block; returns the total */
__device__ inline uint32_t block_exclusive_scan(const uint32_t *in,
                                                uint32_t *out, int64_t n,
                                                ScanT::TempStorage &tmp) {
    const int64_t chunk = (n + SHUF_SCAN_THREADS - 1) / SHUF_SCAN_THREADS;
    int64_t lo = (int64_t)threadIdx.x * chunk;
    if (lo > n) lo = n;
    int64_t hi = lo + chunk;
    if (hi > n) hi = n;
    uint32_t sum = 0;
    for (int64_t i = lo; i < hi; i++) sum += in[i];
    uint32_t pre = 0, total = 0;
    ScanT(tmp).ExclusiveSum(sum, pre, total);
    for (int64_t i = lo; i < hi; i++) {
        const uint32_t v = in[i];
        out[i] = pre;
        pre += v;
    }
    __syncthreads(); /* out[] visible to the block, tmp reusable */
    return total;
}

__global__ void __launch_bounds__(SHUF_SCAN_THREADS)
k_shuf_scan(const uint32_t *hist_rows, const uint32_t *hist_bytes,
            uint32_t *base_rows, uint32_t *base_bytes, int n_parts,
            int n_blocks, int has_utf8, int64_t max_bytes, Starts *st,
            int *err) {
    __shared__ ScanT::TempStorage tmp;
    const int64_t n = (int64_t)n_parts * n_blocks;
    const int tid = threadIdx.x;
    const uint32_t rows = block_exclusive_scan(hist_rows, base_rows, n, tmp);
    if (tid < n_parts) st->row[tid] = base_rows[(int64_t)tid * n_blocks];
    if (tid == n_parts) st->row[tid] = rows;
    if (has_utf8) {
        /* a malformed batch can wrap the sums; nothing reads them then */
        const uint32_t total =
            block_exclusive_scan(hist_bytes, base_bytes, n, tmp);
        if (tid < n_parts) st->byte[tid] = base_bytes[(int64_t)tid * n_blocks];
        if (tid == n_parts) {
            st->byte[tid] = total;
            if ((int64_t)total > max_bytes) atomicMax(err, SHERR_BYTES);
        }
    } else if (tid <= n_parts) {
        st->byte[tid] = 0;
    }
}

__global__ void __launch_bounds__(SHUF_BLOCK)
k_shuf_scatter(ColPtrs C, int n_cols, const int32_t *off, int64_t n_rows,
               int n_parts, const uint8_t *owner, const uint32_t *base_rows,
               int n_blocks, int32_t *len_dst, int32_t *src_dst) {
    /* first the row count, then the destination base, of every
     * (pass, wave, owner) group of this tile */
    __shared__ uint32_t grp[SHUF_PASSES][SHUF_WAVES][AMD_SHUF_MAX_PARTS];
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < SHUF_PASSES * SHUF_WAVES * AMD_SHUF_MAX_PARTS;
         i += SHUF_BLOCK)
        (&grp[0][0][0])[i] = 0;
    __syncthreads();

    const int64_t base = (int64_t)blockIdx.x * SHUF_TILE;
    const unsigned long long below = (1ull << lane) - 1;
    int own[SHUF_PASSES];
    uint32_t rank[SHUF_PASSES];
    for (int it = 0; it < SHUF_PASSES; it++) {
        const int64_t r = base + it * SHUF_BLOCK + tid;
        const bool valid = r < n_rows;
        own[it] = valid ? (int)owner[r] : -1;
        rank[it] = 0;
        /* peel the distinct owners of this wave, lowest lane first; every
         * round retires at least its leader */
        unsigned long long rem = __ballot(valid);
        for (int round = 0; round < 64 && rem; round++) {
            const int leader = __ffsll((long long)rem) - 1;
            const int o = __shfl(own[it], leader);
            const unsigned long long m = __ballot(own[it] == o);
            if (own[it] == o) rank[it] = (uint32_t)__popcll(m & below);
            if (lane == leader) grp[it][wave][o] = (uint32_t)__popcll(m);
            rem &= ~m;
        }
    }
    __syncthreads();
    if (tid < n_parts) {
        uint32_t run = base_rows[(int64_t)tid * n_blocks + blockIdx.x];
        for (int it = 0; it < SHUF_PASSES; it++)
            for (int w = 0; w < SHUF_WAVES; w++) {
                const uint32_t c = grp[it][w][tid];
                grp[it][w][tid] = run;
                run += c;
            }
    }
    __syncthreads();
    for (int it = 0; it < SHUF_PASSES; it++) {
        if (own[it] < 0) break;
        const int64_t r = base + it * SHUF_BLOCK + tid;
        const int64_t d = (int64_t)grp[it][wave][own[it]] + rank[it];
        if (d >= n_rows) continue; /* cannot happen: hist and owner agree */
        for (int c = 0; c < n_cols; c++) C.out[c][d] = C.in[c][r];
        if (off) {
            const int32_t a = off[r];
            len_dst[d] = off[r + 1] - a;
            src_dst[d] = a;
        }
    }
}

/* One wave per (partition p, source block b): its strings are destination
 * rows [base_rows, base_rows + hist_rows) and their bytes start at
 * base_bytes.  Partition p's offsets are written at index row + p, relative
 * to byte_start[p]; the wave of the last block also writes the closing
 * entry. */
__global__ void __launch_bounds__(SHUF_BLOCK)
k_shuf_utf8_offsets(const uint32_t *hist_rows, const uint32_t *base_rows,
                    const uint32_t *base_bytes, int n_parts, int n_blocks,
                    const int32_t *len_dst, const Starts *st,
                    int32_t *out_off, int32_t *pos_dst, const int *err) {
    if (*err) return;
    const int lane = threadIdx.x & 63;
    const int64_t n_runs = (int64_t)n_parts * n_blocks;
    const int64_t stride = (int64_t)gridDim.x * SHUF_WAVES;
    for (int64_t run = (int64_t)blockIdx.x * SHUF_WAVES + (threadIdx.x >> 6);
         run < n_runs; run += stride) {
        const int p = (int)(run / n_blocks);
        const int64_t first = base_rows[run];
        const int64_t count = hist_rows[run];
        const int64_t part_bytes = st->byte[p];
        int64_t pos = base_bytes[run];
        for (int64_t i = 0; i < count; i += 64) {
            const int64_t d = first + i + lane;
            const int32_t len = i + lane < count ? len_dst[d] : 0;
            int32_t incl = len;
            for (int s = 1; s < 64; s <<= 1) {
                const int32_t t = __shfl_up(incl, s);
                if (lane >= s) incl += t;
            }
            if (i + lane < count) {
                const int64_t at = pos + incl - len;
                pos_dst[d] = (int32_t)at;
                out_off[d + p] = (int32_t)(at - part_bytes);
            }
            pos += __shfl(incl, 63);
        }
        if (run % n_blocks == n_blocks - 1 && lane == 0)
            out_off[st->row[p + 1] + p] =
                (int32_t)(st->byte[p + 1] - part_bytes);
    }
}

__device__ inline uint64_t load8(const uint8_t *p) {
    uint64_t w;
    __builtin_memcpy(&w, p, 8);
    return w;
}

__device__ inline void store8(uint8_t *p, uint64_t w) {
    __builtin_memcpy(p, &w, 8);
}

/* One wave per 64 destination rows.  A string of at most `threshold` bytes
 * is copied by its own lane; the longer ones are taken one at a time by the
 * whole wave, 8 bytes a lane.  Reads exactly data[src .. src + len). */
__global__ void __launch_bounds__(SHUF_BLOCK)
k_shuf_utf8_copy(const uint8_t *data, const int32_t *len_dst,
                 const int32_t *src_dst, const int32_t *pos_dst,
                 int64_t n_rows, int32_t threshold, uint8_t *out,
                 const int *err) {
    if (*err) return;
    const int lane = threadIdx.x & 63;
    const int64_t n_groups = (n_rows + 63) / 64;
    const int64_t stride = (int64_t)gridDim.x * SHUF_WAVES;
    for (int64_t g = (int64_t)blockIdx.x * SHUF_WAVES + (threadIdx.x >> 6);
         g < n_groups; g += stride) {
        const int64_t d = g * 64 + lane;
        int32_t len = 0, src = 0, pos = 0;
        if (d < n_rows) {
            len = len_dst[d];
            src = src_dst[d];
            pos = pos_dst[d];
        }
        if (len <= threshold) {
            const uint8_t *s = data + src;
            uint8_t *t = out + pos;
            int32_t i = 0;
            for (; i + 8 <= len; i += 8) store8(t + i, load8(s + i));
            for (; i < len; i++) t[i] = s[i];
        }
        unsigned long long big = __ballot(len > threshold);
        for (int round = 0; round < 64 && big; round++) {
            const int who = __ffsll((long long)big) - 1;
            big &= big - 1;
            const int32_t wlen = __shfl(len, who);
            const uint8_t *s = data + __shfl(src, who);
            uint8_t *t = out + __shfl(pos, who);
            const int32_t body = wlen & ~7;
            for (int32_t i = lane * 8; i < body; i += 512)
                store8(t + i, load8(s + i));
            if (lane < wlen - body) t[body + lane] = s[body + lane];
        }
    }
}

/* n_rows == 0: every partition is an empty Utf8 array, one zero offset */
__global__ void k_shuf_zero_offsets(int32_t *out_off, int n_parts) {
    if ((int)threadIdx.x < n_parts) out_off[threadIdx.x] = 0;
}

}  // namespace shuf

using namespace shuf;

struct GpuShuffle : OpBase {
    AmdShuffleConfig cfg;
    int max_blocks;
    int64_t *out_cols[AMD_SHUF_MAX_COLS];
    uint8_t *owner;
    uint32_t *hist_rows, *hist_bytes, *base_rows, *base_bytes;
    int32_t *len_dst, *src_dst, *pos_dst;
    int32_t *out_off;
    uint8_t *out_data;
    /* where the results go: the buffers above, or the caller's
     * (arroyo_amd_shuffle_bind_output) */
    int64_t *dst_cols[AMD_SHUF_MAX_COLS];
    int32_t *dst_off;
    uint8_t *dst_data;
    Starts *d_starts; /* d_starts->err is the device error word */
    Starts *h_starts; /* pinned */
    int32_t copy_threshold;
    /* opt-in per-kernel timing (arroyo_amd_shuffle_profile) */
    int prof_on;
    hipEvent_t ev[AMD_SHUF_N_KERNELS + 1];
    double last_ms[AMD_SHUF_N_KERNELS];
};

static void shuf_own_output(GpuShuffle *o) {
    for (int c = 0; c < AMD_SHUF_MAX_COLS; c++) o->dst_cols[c] = o->out_cols[c];
    o->dst_off = o->out_off;
    o->dst_data = o->out_data;
}

API void *arroyo_amd_shuffle_create(const AmdShuffleConfig *cfg) {
    if (!cfg || cfg->n_parts < 1 || cfg->n_parts > AMD_SHUF_MAX_PARTS ||
        cfg->n_cols < 1 || cfg->n_cols > AMD_SHUF_MAX_COLS ||
        cfg->key_col < 0 || cfg->key_col >= cfg->n_cols ||
        (cfg->key_mode != AMD_SHUF_KEY_I64 &&
         cfg->key_mode != AMD_SHUF_KEY_HASH) ||
        cfg->max_rows < 1 || cfg->max_rows > AMD_SHUF_MAX_ROWS ||
        (cfg->has_utf8 && (cfg->max_bytes < 0 || cfg->max_bytes > INT32_MAX))) {
        snprintf(g_create_err, sizeof g_create_err,
                 "invalid shuffle config (n_parts 1..%d, n_cols 1..%d, "
                 "key_col < n_cols, key_mode 0/1, max_rows 1..%lld, "
                 "max_bytes 0..INT32_MAX)",
                 AMD_SHUF_MAX_PARTS, AMD_SHUF_MAX_COLS,
                 (long long)AMD_SHUF_MAX_ROWS);
        return nullptr;
    }
    if (hipSetDevice(cfg->device) != hipSuccess) {
        snprintf(g_create_err, sizeof g_create_err,
                 "hipSetDevice(%d) failed: no HIP device (no CPU fallback)",
                 cfg->device);
        return nullptr;
    }
    GpuShuffle *o = new GpuShuffle();
    o->cfg = *cfg;
    o->cfg.has_utf8 = cfg->has_utf8 ? 1 : 0;
    o->copy_threshold = SHUF_COPY_THRESHOLD;
    o->max_blocks = (int)((cfg->max_rows + SHUF_TILE - 1) / SHUF_TILE);
    const size_t rows = (size_t)cfg->max_rows;
    const size_t runs = (size_t)cfg->n_parts * o->max_blocks;
    for (int c = 0; c < cfg->n_cols; c++)
        OP_TRY(o, "shuffle alloc", o->dev_alloc(o->out_cols[c], rows * 8));
    OP_TRY(o, "shuffle alloc", o->dev_alloc(o->owner, rows));
    OP_TRY(o, "shuffle alloc", o->dev_alloc(o->hist_rows, runs * 4));
    OP_TRY(o, "shuffle alloc", o->dev_alloc(o->base_rows, runs * 4));
    OP_TRY(o, "shuffle alloc", o->dev_alloc(o->d_starts, sizeof(Starts)));
    if (o->cfg.has_utf8) {
        OP_TRY(o, "shuffle alloc", o->dev_alloc(o->hist_bytes, runs * 4));
        OP_TRY(o, "shuffle alloc", o->dev_alloc(o->base_bytes, runs * 4));
        OP_TRY(o, "shuffle alloc", o->dev_alloc(o->len_dst, rows * 4));
        OP_TRY(o, "shuffle alloc", o->dev_alloc(o->src_dst, rows * 4));
        OP_TRY(o, "shuffle alloc", o->dev_alloc(o->pos_dst, rows * 4));
        OP_TRY(o, "shuffle alloc",
               o->dev_alloc(o->out_off, (rows + cfg->n_parts) * 4));
        /* max_bytes 0 still gets an address */
        OP_TRY(o, "shuffle alloc",
               o->dev_alloc(o->out_data,
                            cfg->max_bytes ? (size_t)cfg->max_bytes : 1));
    }
    OP_TRY(o, "shuffle alloc", o->pinned_alloc(o->h_starts, sizeof(Starts)));
    OP_TRY(o, "shuffle alloc", o->stream_create(&o->stream));
    shuf_own_output(o);
    return o;
}

API const char *arroyo_amd_shuffle_last_error(void *h) {
    return h ? ((GpuShuffle *)h)->err_msg : g_create_err;
}

API int arroyo_amd_shuffle_bind_output(void *h, int64_t *const *d_out_cols,
                                       int32_t *d_out_offsets,
                                       uint8_t *d_out_data) {
    GpuShuffle *o = (GpuShuffle *)h;
    if (!d_out_cols) {
        shuf_own_output(o);
        return 0;
    }
    for (int c = 0; c < o->cfg.n_cols; c++)
        if (!d_out_cols[c]) {
            snprintf(o->err_msg, sizeof o->err_msg,
                     "bind_output: column %d is NULL", c);
            return 1;
        }
    if (o->cfg.has_utf8 && (!d_out_offsets || !d_out_data)) {
        snprintf(o->err_msg, sizeof o->err_msg,
                 "bind_output: has_utf8 is set but the offsets or data "
                 "buffer is NULL");
        return 1;
    }
    for (int c = 0; c < o->cfg.n_cols; c++) o->dst_cols[c] = d_out_cols[c];
    if (o->cfg.has_utf8) {
        o->dst_off = d_out_offsets;
        o->dst_data = d_out_data;
    }
    return 0;
}

API int arroyo_amd_shuffle_profile(void *h, int enable,
                                   int32_t copy_threshold,
                                   double *last_kernel_ms) {
    GpuShuffle *o = (GpuShuffle *)h;
    if (enable > 0 && !o->ev[0]) {
        HIP_CHECK(o, hipSetDevice(o->cfg.device));
        for (int i = 0; i <= AMD_SHUF_N_KERNELS; i++)
            HIP_CHECK(o, o->event_create(&o->ev[i]));
    }
    if (enable >= 0) o->prof_on = enable > 0;
    if (copy_threshold >= 0) o->copy_threshold = copy_threshold;
    if (last_kernel_ms)
        for (int i = 0; i < AMD_SHUF_N_KERNELS; i++)
            last_kernel_ms[i] = o->last_ms[i];
    return 0;
}

static int shuf_grid(int64_t want_blocks) {
    return (int)(want_blocks > 16384 ? 16384
                                     : (want_blocks < 1 ? 1 : want_blocks));
}

API int arroyo_amd_shuffle_partition_device(void *h,
                                            const int64_t *const *dcols,
                                            const int32_t *d_offsets,
                                            const uint8_t *d_data,
                                            int64_t n_rows,
                                            AmdShuffleOut *out) {
    GpuShuffle *o = (GpuShuffle *)h;
    if (!o) return 1;
    const AmdShuffleConfig &cfg = o->cfg;
    if (!out || !dcols) {
        snprintf(o->err_msg, sizeof o->err_msg, "NULL column array or out");
        return 1;
    }
    if (n_rows < 0 || n_rows > cfg.max_rows) {
        snprintf(o->err_msg, sizeof o->err_msg,
                 "n_rows %lld outside 0..max_rows (%lld)", (long long)n_rows,
                 (long long)cfg.max_rows);
        return 1;
    }
    ColPtrs C;
    memset(&C, 0, sizeof C);
    for (int c = 0; c < cfg.n_cols; c++) {
        /* an empty batch reads no input, so its pointers may be NULL */
        if (n_rows > 0 && !dcols[c]) {
            snprintf(o->err_msg, sizeof o->err_msg, "column %d is NULL", c);
            return 1;
        }
        C.in[c] = dcols[c];
        C.out[c] = o->dst_cols[c];
    }
    if (cfg.has_utf8 && n_rows > 0 && (!d_offsets || !d_data)) {
        snprintf(o->err_msg, sizeof o->err_msg,
                 "has_utf8 is set but the offsets or data pointer is NULL");
        return 1;
    }
    memset(out, 0, sizeof *out);
    out->n_rows = n_rows;
    for (int c = 0; c < cfg.n_cols; c++) out->cols[c] = o->dst_cols[c];
    out->utf8_offsets = o->dst_off;
    out->utf8_data = o->dst_data;
    const int32_t *off = cfg.has_utf8 ? d_offsets : nullptr;
    if (n_rows == 0) {
        /* every partition is an empty Utf8 array: one zero offset each */
        if (cfg.has_utf8) {
            hipLaunchKernelGGL(k_shuf_zero_offsets, dim3(1), dim3(64), 0,
                               o->stream, o->dst_off, cfg.n_parts);
            HIP_CHECK(o, hipGetLastError());
            HIP_CHECK(o, hipStreamSynchronize(o->stream));
        }
        return 0;
    }
    const int nb = (int)((n_rows + SHUF_TILE - 1) / SHUF_TILE);
    int *d_err = (int *)&o->d_starts->err;
    hipEvent_t *ev = o->prof_on ? o->ev : nullptr;
    HIP_CHECK(o, hipMemsetAsync(&o->d_starts->err, 0, 8, o->stream));
    if (ev) HIP_CHECK(o, hipEventRecord(ev[0], o->stream));
    hipLaunchKernelGGL(k_shuf_count, dim3(nb), dim3(SHUF_BLOCK), 0, o->stream,
                       C.in[cfg.key_col], off, n_rows, cfg.n_parts,
                       cfg.key_mode, o->owner, o->hist_rows, o->hist_bytes,
                       nb, d_err);
    if (ev) HIP_CHECK(o, hipEventRecord(ev[1], o->stream));
    hipLaunchKernelGGL(k_shuf_scan, dim3(1), dim3(SHUF_SCAN_THREADS), 0,
                       o->stream, (const uint32_t *)o->hist_rows,
                       (const uint32_t *)o->hist_bytes, o->base_rows,
                       o->base_bytes, cfg.n_parts, nb, cfg.has_utf8,
                       cfg.max_bytes, o->d_starts, d_err);
    if (ev) HIP_CHECK(o, hipEventRecord(ev[2], o->stream));
    hipLaunchKernelGGL(k_shuf_scatter, dim3(nb), dim3(SHUF_BLOCK), 0,
                       o->stream, C, cfg.n_cols, off, n_rows, cfg.n_parts,
                       (const uint8_t *)o->owner,
                       (const uint32_t *)o->base_rows, nb, o->len_dst,
                       o->src_dst);
    if (ev) HIP_CHECK(o, hipEventRecord(ev[3], o->stream));
    if (off) {
        const int64_t runs = (int64_t)cfg.n_parts * nb;
        hipLaunchKernelGGL(k_shuf_utf8_offsets,
                           dim3(shuf_grid((runs + SHUF_WAVES - 1) / SHUF_WAVES)),
                           dim3(SHUF_BLOCK), 0, o->stream,
                           (const uint32_t *)o->hist_rows,
                           (const uint32_t *)o->base_rows,
                           (const uint32_t *)o->base_bytes, cfg.n_parts, nb,
                           (const int32_t *)o->len_dst,
                           (const Starts *)o->d_starts, o->dst_off,
                           o->pos_dst, (const int *)d_err);
        if (ev) HIP_CHECK(o, hipEventRecord(ev[4], o->stream));
        hipLaunchKernelGGL(k_shuf_utf8_copy,
                           dim3(shuf_grid((n_rows + SHUF_BLOCK - 1) / SHUF_BLOCK)),
                           dim3(SHUF_BLOCK), 0, o->stream, d_data,
                           (const int32_t *)o->len_dst,
                           (const int32_t *)o->src_dst,
                           (const int32_t *)o->pos_dst, n_rows,
                           o->copy_threshold, o->dst_data,
                           (const int *)d_err);
        if (ev) HIP_CHECK(o, hipEventRecord(ev[5], o->stream));
    }
    HIP_CHECK(o, hipGetLastError());
    HIP_CHECK(o, hipMemcpyAsync(o->h_starts, o->d_starts, sizeof(Starts),
                               hipMemcpyDeviceToHost, o->stream));
    HIP_CHECK(o, hipStreamSynchronize(o->stream));
    if (ev) {
        const int n_ev = off ? AMD_SHUF_N_KERNELS : 3;
        for (int i = 0; i < AMD_SHUF_N_KERNELS; i++) {
            float ms = 0.f;
            if (i < n_ev)
                HIP_CHECK(o, hipEventElapsedTime(&ms, ev[i], ev[i + 1]));
            o->last_ms[i] = ms;
        }
    }
    const int err = (int)o->h_starts->err;
    if (err == SHERR_OFFSETS) {
        snprintf(o->err_msg, sizeof o->err_msg,
                 "malformed offsets: negative or decreasing");
        return 1;
    }
    if (err == SHERR_BYTES) {
        snprintf(o->err_msg, sizeof o->err_msg,
                 "Utf8 column holds %lld bytes, above max_bytes (%lld)",
                 (long long)o->h_starts->byte[cfg.n_parts],
                 (long long)cfg.max_bytes);
        return 1;
    }
    for (int p = 0; p <= cfg.n_parts; p++) {
        out->row_start[p] = o->h_starts->row[p];
        out->byte_start[p] = o->h_starts->byte[p];
    }
    return 0;
}

API void arroyo_amd_shuffle_destroy(void *h) {
    delete (GpuShuffle *)h;   /* ~OpBase drains the stream first */
}
