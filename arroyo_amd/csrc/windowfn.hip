/* arroyo-amd SQL window function (ROW_NUMBER per instant): MI355X-native
 * (gfx950) equivalent of WindowFunctionOperator
 * (crates/arroyo-worker/src/arrow/window_fn.rs) behind the
 * arroyo_amd_windowfn_* C ABI (include/arroyo_amd.h).
 *
 * MI355X-first design (NOT a translation of the reference's per-instant
 * DataFusion BoundedWindowAggExec streams):
 *   - rows land in a device-resident instant table (open-addressed by exact
 *     `_timestamp`, append planes with wave-aggregated cursors, late rows
 *     silently filtered -- filter_and_split_batches :52-93);
 *   - on watermark, instants < wm fire in timestamp order: the instant's
 *     rows are gathered contiguous, a permutation is built with stable
 *     hipCUB radix sorts (least-significant ORDER BY column first, then the
 *     PARTITION BY column; i64 keys order-encoded into u64, descending via
 *     complement -- ties therefore resolve to input order exactly like
 *     DataFusion's stable sort), ROW_NUMBER is a head-flag inclusive scan,
 *     and the downstream `row_number <= limit` filter is fused into the
 *     emit kernel so the full ranking is never materialised.
 *
 * Parity is pinned against oracle/arroyo_oracle.c (itself pinned against
 * the reference's most_active_driver_last_hour golden vector) by
 * tests/test_windowfn.py.
 */
#include <hipcub/hipcub.hpp>

#include <map>

#include "op_common.h"

namespace wfn {

#define WERR_INSTANTS 1
#define WERR_ROWS_CAP 2
#define WERR_OUT_CAP  3

__device__ inline uint64_t enc_asc(int64_t v) {
    return ((uint64_t)v) ^ 0x8000000000000000ULL;
}

/* claim-or-find the slot for instant t */
__device__ inline int32_t wf_claim(uint64_t *tag, uint32_t I, uint64_t t,
                                   int *err) {
    uint32_t m = I - 1;
    uint32_t j = (uint32_t)hash64(t) & m;
    for (uint32_t probes = 0; probes < I; probes++) {
        uint64_t cur = tag[j];
        if (cur == t) return (int32_t)j;
        if (cur == EMPTY_TAG) {
            uint64_t old = atomicCAS((unsigned long long *)&tag[j],
                                     (unsigned long long)EMPTY_TAG,
                                     (unsigned long long)t);
            if (old == EMPTY_TAG || old == t) return (int32_t)j;
        }
        j = (j + 1) & m;
    }
    *err = WERR_INSTANTS;
    return -1;
}

struct WfAppendArgs {
    const int64_t *cols[12];
    int32_t n_cols;           /* incl trailing ts */
    int64_t n_rows;
    uint64_t *tag;
    unsigned long long *cursor;
    int64_t *planes;          /* [n_cols][I*cap]; last = arrival seq */
    uint32_t I, cap;
    int has_wm; uint64_t wm;
    int64_t seq_base;         /* rows processed before this batch */
    int *err;
};

__global__ void __launch_bounds__(256)
k_wf_append(WfAppendArgs A) {
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t *ts = A.cols[A.n_cols - 1];
    size_t plane = (size_t)A.I * A.cap;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         i < A.n_rows; i += stride) {
        uint64_t t = (uint64_t)ts[i];
        if (A.has_wm && t < A.wm) continue;  /* late: silently filtered */
        int32_t slot = wf_claim(A.tag, A.I, t, A.err);
        if (slot < 0) continue;
        uint64_t idx = atomicAdd(&A.cursor[slot], 1ULL);
        if (idx >= A.cap) { *A.err = WERR_ROWS_CAP; continue; }
        size_t off = (size_t)slot * A.cap + idx;
        for (int c = 0; c < A.n_cols - 1; c++)
            A.planes[(size_t)c * plane + off] = A.cols[c][i];
        /* arrival order, so ROW_NUMBER ties resolve exactly like the
         * reference's stable sort regardless of append-kernel scheduling */
        A.planes[(size_t)(A.n_cols - 1) * plane + off] = A.seq_base + i;
    }
}

/* gather one instant group's rows (possibly several table slots after slot
 * recycling) into contiguous scratch columns */
__global__ void __launch_bounds__(256)
k_wf_gather(const int64_t *planes, size_t plane, uint32_t cap, int n_data,
            const uint32_t *slots, const int64_t *slot_off, int n_slots,
            int64_t total, int64_t *scratch, int64_t scap) {
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         i < total; i += stride) {
        int s = 0;
        while (i >= slot_off[s + 1]) s++;
        size_t off = (size_t)slots[s] * cap + (i - slot_off[s]);
        for (int c = 0; c < n_data; c++)
            scratch[(size_t)c * scap + i] = planes[(size_t)c * plane + off];
    }
}

__global__ void __launch_bounds__(256)
k_wf_keys(const int64_t *col, const int64_t *perm, uint64_t *keys,
          int64_t n, int desc) {
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         i < n; i += stride) {
        uint64_t k = enc_asc(col[perm[i]]);
        keys[i] = desc ? ~k : k;
    }
}

__global__ void __launch_bounds__(256)
k_wf_iota(int64_t *perm, int64_t n) {
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         i < n; i += stride)
        perm[i] = i;
}

__global__ void __launch_bounds__(256)
k_wf_heads(const int64_t *part, const int64_t *perm, int64_t *hf, int64_t n,
           int has_part) {
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         i < n; i += stride)
        hf[i] = i == 0 ||
                (has_part && part[perm[i]] != part[perm[i - 1]]);
}

__global__ void __launch_bounds__(256)
k_wf_segstart(const int64_t *hf, const int64_t *segid, int64_t *segstart,
              int64_t n) {
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         i < n; i += stride)
        if (hf[i]) segstart[segid[i] - 1] = i;
}

struct WfEmitArgs {
    const int64_t *scratch;   /* [n_data][scap] */
    int64_t scap;
    const int64_t *perm;
    const int64_t *segid;
    const int64_t *segstart;
    int64_t n;
    int n_data;
    int64_t limit;
    uint64_t instant;
    int64_t *out[14];
    unsigned long long *n_out;
    int64_t out_cap;
    int *err;
};

__global__ void __launch_bounds__(256)
k_wf_emit(WfEmitArgs E) {
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         i < E.n; i += stride) {
        int64_t rn = i - E.segstart[E.segid[i] - 1] + 1;
        if (E.limit && rn > E.limit) continue;
        int64_t r = (int64_t)atomicAdd(E.n_out, 1ULL);
        if (r >= E.out_cap) { *E.err = WERR_OUT_CAP; continue; }
        for (int c = 0; c < E.n_data; c++)
            E.out[c][r] = E.scratch[(size_t)c * E.scap + E.perm[i]];
        E.out[E.n_data][r] = (int64_t)E.instant;
        E.out[E.n_data + 1][r] = rn;
    }
}

}  // namespace wfn

using namespace wfn;

struct GpuWindowFn : OpBase {
    AmdWindowFnConfig cfg;
    int64_t seq;
    uint32_t I, cap;
    int n_data;               /* n_cols - 1 */
    uint64_t *tag;
    unsigned long long *cursor;
    int64_t *planes;
    /* fire scratch */
    int64_t scap;
    int64_t *scratch;
    int64_t *perm, *perm2;
    uint64_t *keys, *keys2;
    int64_t *hf, *segid, *segstart;
    void *cub_tmp;
    size_t cub_bytes;
    uint32_t *d_slots;
    int64_t *d_slot_off;
    int64_t *d_out[14];
    unsigned long long *d_n_out;
    int64_t out_cap;
    Staging stg;
    std::vector<std::vector<int64_t>> host_out;
    int out_cols;
    int has_wm; uint64_t wm;
};

API void *arroyo_amd_windowfn_create(const AmdWindowFnConfig *cfg) {
    if (!cfg || cfg->n_cols < 2 || cfg->n_cols > 12 || cfg->n_order < 1 ||
        cfg->n_order > 2 || cfg->part_col >= cfg->n_cols - 1) {
        snprintf(g_create_err, sizeof g_create_err, "invalid windowfn config");
        return nullptr;
    }
    GpuWindowFn *o = new GpuWindowFn();
    o->cfg = *cfg;
    o->I = cfg->instants ? cfg->instants : 128;
    o->cap = 1u << (cfg->log2_rows_cap ? cfg->log2_rows_cap : 15);
    o->n_data = cfg->n_cols - 1;
    o->out_cols = cfg->n_cols + 1;
    o->out_cap = 1ll << (cfg->log2_out_cap ? cfg->log2_out_cap : 20);
    if (hipSetDevice(cfg->device) != hipSuccess) {
        snprintf(g_create_err, sizeof g_create_err,
                 "hipSetDevice(%d) failed: no HIP device (no CPU fallback)",
                 cfg->device);
        delete o;
        return nullptr;
    }
    size_t plane = (size_t)o->I * o->cap;
    o->scap = (int64_t)plane;
    OP_ALLOC(o, o->tag, (size_t)o->I * 8, 0xFF);
    OP_ALLOC(o, o->cursor, (size_t)o->I * 8, 0);
    OP_ALLOC(o, o->planes, ((size_t)o->n_data + 1) * plane * 8);
    OP_ALLOC(o, o->scratch, ((size_t)o->n_data + 1) * plane * 8);
    OP_ALLOC(o, o->perm, plane * 8);
    OP_ALLOC(o, o->perm2, plane * 8);
    OP_ALLOC(o, o->keys, plane * 8);
    OP_ALLOC(o, o->keys2, plane * 8);
    OP_ALLOC(o, o->hf, plane * 8);
    OP_ALLOC(o, o->segid, plane * 8);
    OP_ALLOC(o, o->segstart, plane * 8);
    OP_ALLOC(o, o->d_slots, 64 * 4);
    OP_ALLOC(o, o->d_slot_off, 65 * 8);
    for (int i = 0; i < o->out_cols; i++)
        OP_ALLOC(o, o->d_out[i], (size_t)o->out_cap * 8);
    OP_ALLOC(o, o->d_n_out, 8);
    OP_ALLOC(o, o->d_err, 4, 0);
    /* hipCUB temp sizing (worst case n = plane) */
    o->cub_bytes = 0;
    OP_TRY(o, "cub sort size",
           hipcub::DeviceRadixSort::SortPairs(nullptr, o->cub_bytes, o->keys,
                                              o->keys2, o->perm, o->perm2,
                                              (int)plane));
    size_t scan_bytes = 0;
    OP_TRY(o, "cub scan size",
           hipcub::DeviceScan::InclusiveSum(nullptr, scan_bytes, o->hf,
                                            o->segid, (int)plane));
    if (scan_bytes > o->cub_bytes) o->cub_bytes = scan_bytes;
    OP_TRY_MSG(o, "cub temp alloc failed",
               o->dev_alloc(o->cub_tmp, o->cub_bytes ? o->cub_bytes : 1));
    OP_TRY(o, "hipStreamCreate", o->stream_create(&o->stream));
    OP_TRY_MSG(o, "windowfn staging alloc failed",
               o->stg.alloc(o, cfg->n_cols, 1 << 20));
    o->host_out.resize(o->out_cols);
    return o;
}

API const char *arroyo_amd_windowfn_last_error(void *h) {
    return h ? ((GpuWindowFn *)h)->err_msg : g_create_err;
}

static const char *wf_err_msg(int e) {
    return e == WERR_INSTANTS ? "live-instant table full; raise instants"
           : e == WERR_ROWS_CAP
               ? "per-instant row buffer full; raise log2_rows_cap"
           : e == WERR_OUT_CAP ? "output buffer full; raise log2_out_cap"
                               : "device error";
}

/* append n_rows device rows to the instant table, stamping arrival order */
static int wf_append(GpuWindowFn *o, const int64_t *const *dcols,
                     int32_t n_cols, int64_t n_rows) {
    WfAppendArgs A = {};
    for (int c = 0; c < n_cols; c++) A.cols[c] = dcols[c];
    A.n_cols = n_cols;
    A.n_rows = n_rows;
    A.tag = o->tag;
    A.cursor = o->cursor;
    A.planes = o->planes;
    A.I = o->I;
    A.cap = o->cap;
    A.has_wm = o->has_wm;
    A.wm = o->wm;
    A.seq_base = o->seq;
    o->seq += n_rows;
    A.err = o->d_err;
    hipLaunchKernelGGL(k_wf_append, dim3(grid_for(n_rows, 2048)), dim3(256),
                       0, o->stream, A);
    HIP_CHECK(o, hipGetLastError());
    return 0;
}

static int wf_check_cols(GpuWindowFn *o, int32_t n_cols) {
    if (n_cols == o->cfg.n_cols) return 0;
    snprintf(o->err_msg, sizeof o->err_msg, "expected %d cols, got %d",
             o->cfg.n_cols, n_cols);
    return 1;
}

API int arroyo_amd_windowfn_process_batch(void *h, const int64_t *const *cols,
                                          int32_t n_cols, int64_t n_rows) {
    GpuWindowFn *o = (GpuWindowFn *)h;
    if (wf_check_cols(o, n_cols)) return 1;
    int64_t done = 0;
    while (done < n_rows) {
        int64_t take = n_rows - done;
        if (take > o->stg.cap) take = o->stg.cap;
        const int64_t *dcols[12];
        if (o->stg.stage_chunk(o, cols, n_cols, done, take, dcols) ||
            wf_append(o, dcols, n_cols, take))
            return 1;
        /* staging reused next iteration: wait for this append to finish */
        HIP_CHECK(o, hipStreamSynchronize(o->stream));
        done += take;
    }
    return 0;
}

/* device-resident ingest: rows already in HBM append straight into the
 * instant table (no host staging); same arrival-sequence stamping */
API int arroyo_amd_windowfn_process_batch_device(void *h,
                                                 const int64_t *const *dcols,
                                                 int32_t n_cols,
                                                 int64_t n_rows) {
    GpuWindowFn *o = (GpuWindowFn *)h;
    if (wf_check_cols(o, n_cols)) return 1;
    return wf_append(o, dcols, n_cols, n_rows);
}

/* one stable radix pass: reorder perm by scratch column `col` of the n
 * gathered rows */
static int wf_sort_pass(GpuWindowFn *o, int col, int desc, int64_t n) {
    hipLaunchKernelGGL(k_wf_keys, dim3(grid_for(n, 2048)), dim3(256), 0,
                       o->stream, o->scratch + (size_t)col * o->scap, o->perm,
                       o->keys, n, desc);
    HIP_CHECK(o, hipGetLastError());
    size_t tmp = o->cub_bytes;
    HIP_CHECK(o, hipcub::DeviceRadixSort::SortPairs(
                     o->cub_tmp, tmp, o->keys, o->keys2, o->perm, o->perm2,
                     (int)n, 0, 64, o->stream));
    std::swap(o->perm, o->perm2);
    return 0;
}

static int wf_fire(GpuWindowFn *o, uint64_t instant,
                   const std::vector<uint32_t> &slots,
                   const std::vector<unsigned long long> &cnt) {
    const AmdWindowFnConfig &c = o->cfg;
    size_t plane = (size_t)o->I * o->cap;
    std::vector<int64_t> off(slots.size() + 1, 0);
    std::vector<uint32_t> sl(slots);
    for (size_t i = 0; i < slots.size(); i++) {
        int64_t c_i = (int64_t)cnt[slots[i]];
        if (c_i > (int64_t)o->cap) c_i = o->cap;  /* overflow already err'd */
        off[i + 1] = off[i] + c_i;
    }
    int64_t n = off.back();
    if (n == 0) {
        for (uint32_t s : slots) {
            HIP_CHECK(o, hipMemsetAsync(o->tag + s, 0xFF, 8, o->stream));
            HIP_CHECK(o, hipMemsetAsync(o->cursor + s, 0, 8, o->stream));
        }
        return 0;
    }
    HIP_CHECK(o, hipMemcpyAsync(o->d_slots, sl.data(), sl.size() * 4,
                                hipMemcpyHostToDevice, o->stream));
    HIP_CHECK(o, hipMemcpyAsync(o->d_slot_off, off.data(), off.size() * 8,
                                hipMemcpyHostToDevice, o->stream));
    hipLaunchKernelGGL(k_wf_gather, dim3(grid_for(n, 2048)), dim3(256), 0,
                       o->stream, o->planes, plane, o->cap, o->n_data + 1,
                       o->d_slots, o->d_slot_off, (int)sl.size(), n,
                       o->scratch, o->scap);
    HIP_CHECK(o, hipGetLastError());
    hipLaunchKernelGGL(k_wf_iota, dim3(grid_for(n, 2048)),
                       dim3(256), 0, o->stream,
                       o->perm, n);
    HIP_CHECK(o, hipGetLastError());
    /* stable radix passes, least significant first: arrival seq (makes
     * ties deterministic = input order, like the reference's stable sort),
     * then ORDER BY cols, then the partition col */
    if (wf_sort_pass(o, o->n_data, 0, n)) return 1;
    for (int j = c.n_order - 1; j >= 0; j--)
        if (wf_sort_pass(o, c.order_col[j], c.order_desc[j], n)) return 1;
    if (c.part_col >= 0 && wf_sort_pass(o, c.part_col, 0, n)) return 1;
    hipLaunchKernelGGL(k_wf_heads, dim3(grid_for(n, 2048)),
                       dim3(256), 0, o->stream,
                       c.part_col >= 0
                           ? o->scratch + (size_t)c.part_col * o->scap
                           : o->scratch,
                       o->perm, o->hf, n, c.part_col >= 0 ? 1 : 0);
    HIP_CHECK(o, hipGetLastError());
    size_t tmp = o->cub_bytes;
    HIP_CHECK(o, hipcub::DeviceScan::InclusiveSum(o->cub_tmp, tmp, o->hf,
                                                  o->segid, (int)n,
                                                  o->stream));
    hipLaunchKernelGGL(k_wf_segstart, dim3(grid_for(n, 2048)), dim3(256), 0,
                       o->stream, o->hf, o->segid, o->segstart, n);
    HIP_CHECK(o, hipGetLastError());
    WfEmitArgs E = {};
    E.scratch = o->scratch;
    E.scap = o->scap;
    E.perm = o->perm;
    E.segid = o->segid;
    E.segstart = o->segstart;
    E.n = n;
    E.n_data = o->n_data;
    E.limit = c.limit;
    E.instant = instant;
    for (int i = 0; i < o->out_cols; i++) E.out[i] = o->d_out[i];
    E.n_out = o->d_n_out;
    E.out_cap = o->out_cap;
    E.err = o->d_err;
    hipLaunchKernelGGL(k_wf_emit, dim3(grid_for(n, 2048)),
                       dim3(256), 0, o->stream,
                       E);
    HIP_CHECK(o, hipGetLastError());
    /* retire the group's slots */
    for (uint32_t s : slots) {
        HIP_CHECK(o, hipMemsetAsync(o->tag + s, 0xFF, 8, o->stream));
        HIP_CHECK(o, hipMemsetAsync(o->cursor + s, 0, 8, o->stream));
    }
    return 0;
}

API int arroyo_amd_windowfn_handle_watermark(void *h, uint64_t wm,
                                             AmdOutBatch *out) {
    GpuWindowFn *o = (GpuWindowFn *)h;
    if (op_check_err(o, wf_err_msg)) return 1;
    o->has_wm = 1;
    o->wm = wm;
    std::vector<uint64_t> tags(o->I);
    std::vector<unsigned long long> cnt(o->I);
    HIP_CHECK(o, hipMemcpyAsync(tags.data(), o->tag, (size_t)o->I * 8,
                                hipMemcpyDeviceToHost, o->stream));
    HIP_CHECK(o, hipMemcpyAsync(cnt.data(), o->cursor, (size_t)o->I * 8,
                                hipMemcpyDeviceToHost, o->stream));
    HIP_CHECK(o, hipStreamSynchronize(o->stream));
    HIP_CHECK(o, hipMemsetAsync(o->d_n_out, 0, 8, o->stream));
    std::map<uint64_t, std::vector<uint32_t>> fired;
    for (uint32_t s = 0; s < o->I; s++)
        if (tags[s] != EMPTY_TAG && tags[s] < wm) fired[tags[s]].push_back(s);
    for (auto &kv : fired)
        if (wf_fire(o, kv.first, kv.second, cnt)) return 1;
    unsigned long long n = 0;
    HIP_CHECK(o, hipMemcpyAsync(&n, o->d_n_out, 8, hipMemcpyDeviceToHost,
                                o->stream));
    HIP_CHECK(o, hipStreamSynchronize(o->stream));
    if (op_check_err(o, wf_err_msg)) return 1;
    if (out) {
        if (op_out_alloc(o, out, (int64_t)n, o->out_cols, __func__)) return 1;
        if (out_copy_cols(o, out, o->d_out, (int64_t)n)) return 1;
    }
    return 0;
}

/* restore = re-ingest the drained rows (state IS the raw buffered rows;
 * drain preserves per-instant arrival order so fresh sequence stamps
 * reproduce the ROW_NUMBER tiebreak), mirroring the reference's
 * buffered-instant table restore (window_fn.rs ExpiringTimeKeyTable). */
API int arroyo_amd_windowfn_restore(void *h, const int64_t *const *cols,
                                    int32_t n_cols, int64_t n_rows) {
    return arroyo_amd_windowfn_process_batch(h, cols, n_cols, n_rows);
}

API int arroyo_amd_windowfn_checkpoint_drain(void *h, AmdOutBatch *out) {
    GpuWindowFn *o = (GpuWindowFn *)h;
    if (op_check_err(o, wf_err_msg)) return 1;
    std::vector<uint64_t> tags(o->I);
    std::vector<unsigned long long> cnt(o->I);
    HIP_CHECK(o, hipMemcpyAsync(tags.data(), o->tag, (size_t)o->I * 8,
                                hipMemcpyDeviceToHost, o->stream));
    HIP_CHECK(o, hipMemcpyAsync(cnt.data(), o->cursor, (size_t)o->I * 8,
                                hipMemcpyDeviceToHost, o->stream));
    HIP_CHECK(o, hipStreamSynchronize(o->stream));
    int ncols = o->cfg.n_cols;
    int64_t total = 0;
    for (uint32_t s = 0; s < o->I; s++)
        if (tags[s] != EMPTY_TAG) total += (int64_t)cnt[s];
    if (op_out_alloc(o, out, total, ncols, __func__)) return 1;
    size_t plane = (size_t)o->I * o->cap;
    int64_t r = 0;
    for (uint32_t s = 0; s < o->I; s++) {
        if (tags[s] == EMPTY_TAG || cnt[s] == 0) continue;
        int64_t n = (int64_t)cnt[s];
        for (int cdx = 0; cdx < ncols - 1; cdx++)
            HIP_CHECK(o, hipMemcpyAsync(
                    (int64_t *)out->cols[cdx] + r,
                    o->planes + (size_t)cdx * plane + (size_t)s * o->cap,
                    (size_t)n * 8, hipMemcpyDeviceToHost, o->stream));
        HIP_CHECK(o, hipStreamSynchronize(o->stream));
        for (int64_t j = 0; j < n; j++)
            ((int64_t *)out->cols[ncols - 1])[r + j] = (int64_t)tags[s];
        r += n;
    }
    return 0;
}

API void arroyo_amd_windowfn_destroy(void *h) {
    delete (GpuWindowFn *)h;   /* ~OpBase drains the stream first */
}
