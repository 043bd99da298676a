/* arroyo-amd SQL window functions (per instant): MI355X-native
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
 *     emit kernel so the full ranking is never materialised;
 *   - the other functions (AmdWindowFnConfig.fn: RANK, DENSE_RANK, LAG,
 *     LEAD, FIRST/LAST_VALUE, SUM, COUNT, MIN, MAX) share the sort and
 *     then take a path of their own: partition and peer-group heads are
 *     flagged together and numbered by one packed inclusive sum, SUM / MIN
 *     / MAX run a three-launch segmented scan (k_wf_scan_*), and without a
 *     limit every row's output place is its sorted position, so the
 *     output order is the sort order and the validity bitmap of LAG/LEAD
 *     is one __ballot per wave.
 *
 * Parity is pinned against oracle/arroyo_oracle.c (itself pinned against
 * the reference's most_active_driver_last_hour golden vector) by
 * tests/test_windowfn.py; the functions beyond ROW_NUMBER, which the oracle
 * lacks, against the independent restatement tests/windowfn_ref.py by
 * tests/test_windowfn_funcs.py.
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

/* ------------------------------------------------------------------ */
/* functions beyond ROW_NUMBER (cfg.fn != 0): everything below runs    */
/* only for them                                                       */

/* partition-head flag in bit 32, peer-head flag in bit 0: one inclusive
 * sum of the packed word numbers partitions (high half) and peer groups
 * (low half, counted across the instant) from 1; n < 2^31 keeps the low
 * half from carrying */
__global__ void __launch_bounds__(256)
k_wf_flags(const int64_t *part, const int64_t *o0, const int64_t *o1,
           const int64_t *perm, int64_t *hf, int64_t n) {
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         i < n; i += stride) {
        int64_t ph = 1, gh = 1;
        if (i > 0) {
            int64_t a = perm[i], b = perm[i - 1];
            ph = part && part[a] != part[b];
            gh = ph || o0[a] != o0[b] || (o1 && o1[a] != o1[b]);
        }
        hf[i] = (ph << 32) | gh;
    }
}

/* first sorted position of every partition and peer group, by id - 1, and
 * one entry past the last id holding n: a group ends where the next one
 * starts.  Both tables hold n + 1 entries at least. */
__global__ void __launch_bounds__(256)
k_wf_starts(const int64_t *hf, const int64_t *ids, int64_t *pstart,
            int64_t *gstart, int64_t n) {
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         i < n; i += stride) {
        int64_t pid = ids[i] >> 32, gid = ids[i] & 0xffffffffLL;
        if (hf[i] >> 32) pstart[pid - 1] = i;
        if (hf[i] & 1) gstart[gid - 1] = i;
        if (i == n - 1) {
            pstart[pid] = n;
            gstart[gid] = n;
        }
    }
}

/* Segmented inclusive scan of arg (read through perm) under the partition
 * head flags: reduce each tile to a (flag, value) partial, scan the
 * partials in one block, then scan each tile again seeded with the
 * partial before it.  Three launches in stream order; no block ever waits
 * for another. */
#define WFN_IPT (AMD_WFN_SCAN_TILE / 256)   /* consecutive rows per thread */

enum { SOP_ADD, SOP_MIN, SOP_MAX };

template <int OP>
__device__ inline int64_t sop_identity() {
    return OP == SOP_ADD ? 0 : OP == SOP_MIN ? INT64_MAX : INT64_MIN;
}

template <int OP>
__device__ inline int64_t sop(int64_t a, int64_t b) {
    if (OP == SOP_ADD) return (int64_t)((uint64_t)a + (uint64_t)b);
    if (OP == SOP_MIN) return a < b ? a : b;
    return a > b ? a : b;
}

struct FV {
    int f;          /* a segment starts somewhere in the span */
    int64_t v;      /* op over the span's rows from its last start on */
};

/* a then b, b to the right of a */
template <int OP>
__device__ inline FV seg_op(FV a, FV b) {
    FV r;
    r.f = a.f | b.f;
    r.v = b.f ? b.v : sop<OP>(a.v, b.v);
    return r;
}

/* One (flag, value) per thread of a 256-thread block, every thread
 * calling: returns the combination of the threads before this one and
 * sets *total to the block's.  __shfl_up ladder inside a wave of 64, the
 * four wave totals through LDS. */
template <int OP>
__device__ inline FV block_exscan(FV x, int *s_f, int64_t *s_v, FV *total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    FV inc = x;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        FV u;
        u.f = __shfl_up(inc.f, d);
        u.v = (int64_t)__shfl_up((long long)inc.v, d);
        if (lane >= d) inc = seg_op<OP>(u, inc);
    }
    if (lane == 63) {
        s_f[w] = inc.f;
        s_v[w] = inc.v;
    }
    FV prev;
    prev.f = __shfl_up(inc.f, 1);
    prev.v = (int64_t)__shfl_up((long long)inc.v, 1);
    __syncthreads();
    FV ex = {0, sop_identity<OP>()}, tot = ex;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        FV wk = {s_f[k], s_v[k]};
        if (k < w) ex = seg_op<OP>(ex, wk);
        tot = seg_op<OP>(tot, wk);
    }
    if (lane > 0) ex = seg_op<OP>(ex, prev);
    *total = tot;
    __syncthreads();   /* the wave totals may be overwritten from here on */
    return ex;
}

struct WfScanArgs {
    const int64_t *arg;       /* scratch column */
    const int64_t *perm;
    const int64_t *hf;        /* packed flags; bit 32 = partition head */
    int64_t n;
    int64_t n_tiles;
    int *pf;                  /* [n_tiles] tile partials ... */
    int64_t *pv;              /* ... whose values k_wf_scan_partials turns
                                 into the inclusive scan over tiles */
    int64_t *out;             /* [n] */
};

/* this thread's WFN_IPT consecutive rows of tile `tile` (identity past n)
 * and their combination */
template <int OP>
__device__ inline FV tile_load(const WfScanArgs &S, int64_t tile,
                               FV it[WFN_IPT]) {
    int64_t base = tile * AMD_WFN_SCAN_TILE + (int64_t)threadIdx.x * WFN_IPT;
    FV agg = {0, sop_identity<OP>()};
#pragma unroll
    for (int j = 0; j < WFN_IPT; j++) {
        int64_t i = base + j;
        it[j] = FV{0, sop_identity<OP>()};
        if (i < S.n) {
            it[j].f = (int)(S.hf[i] >> 32);
            it[j].v = S.arg[S.perm[i]];
        }
        agg = seg_op<OP>(agg, it[j]);
    }
    return agg;
}

template <int OP>
__global__ void __launch_bounds__(256)
k_wf_scan_reduce(WfScanArgs S) {
    __shared__ int s_f[4];
    __shared__ int64_t s_v[4];
    FV it[WFN_IPT], tot;
    FV agg = tile_load<OP>(S, blockIdx.x, it);
    block_exscan<OP>(agg, s_f, s_v, &tot);
    if (threadIdx.x == 0) {
        S.pf[blockIdx.x] = tot.f;
        S.pv[blockIdx.x] = tot.v;
    }
}

/* one block: inclusive scan of the tile partials, 256 at a time with the
 * carry in registers; pv[b] becomes the scan value at the end of tile b */
template <int OP>
__global__ void __launch_bounds__(256)
k_wf_scan_partials(WfScanArgs S) {
    __shared__ int s_f[4];
    __shared__ int64_t s_v[4];
    FV carry = {0, sop_identity<OP>()};
    for (int64_t base = 0; base < S.n_tiles; base += 256) {
        int64_t b = base + threadIdx.x;
        FV x = {0, sop_identity<OP>()}, tot;
        if (b < S.n_tiles) {
            x.f = S.pf[b];
            x.v = S.pv[b];
        }
        FV ex = block_exscan<OP>(x, s_f, s_v, &tot);
        if (b < S.n_tiles)
            S.pv[b] = seg_op<OP>(seg_op<OP>(carry, ex), x).v;
        carry = seg_op<OP>(carry, tot);
    }
}

template <int OP>
__global__ void __launch_bounds__(256)
k_wf_scan_down(WfScanArgs S) {
    __shared__ int s_f[4];
    __shared__ int64_t s_v[4];
    FV it[WFN_IPT], tot;
    FV agg = tile_load<OP>(S, blockIdx.x, it);
    FV run = {0, blockIdx.x ? S.pv[blockIdx.x - 1] : sop_identity<OP>()};
    run = seg_op<OP>(run, block_exscan<OP>(agg, s_f, s_v, &tot));
    int64_t base = (int64_t)blockIdx.x * AMD_WFN_SCAN_TILE +
                   (int64_t)threadIdx.x * WFN_IPT;
#pragma unroll
    for (int j = 0; j < WFN_IPT; j++) {
        run = seg_op<OP>(run, it[j]);
        if (base + j < S.n) S.out[base + j] = run.v;
    }
}

struct WfFnArgs {
    const int64_t *scratch;   /* [n_data][scap] */
    int64_t scap;
    const int64_t *perm;
    const int64_t *ids;       /* partition id << 32 | peer-group id */
    const int64_t *pstart, *gstart;
    const int64_t *scan;      /* SUM MIN MAX: the segmented scan */
    const int64_t *arg;       /* scratch column, or null */
    int64_t n;
    int n_data;
    int fn, frame;
    int64_t k;
    int has_default;
    int64_t default_value;
    int64_t limit;
    uint64_t instant;
    int64_t *out[14];
    int64_t base;             /* limit == 0: output row = base + position */
    unsigned long long *n_out;   /* limit != 0: the output cursor */
    int64_t out_cap;
    int *err;
    unsigned long long *vbits;   /* validity of the function column, one
                                    word per 64 positions; null = unwanted */
};

/* every wave takes 64 consecutive sorted positions, so one __ballot is one
 * word of the validity plane: no atomics touch it */
__global__ void __launch_bounds__(256)
k_wf_emit_fn(WfFnArgs E) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int lane = threadIdx.x & 63;
    for (int64_t wbase = (int64_t)blockIdx.x * blockDim.x +
                         (threadIdx.x - lane);
         wbase < E.n; wbase += stride) {
        const int64_t i = wbase + lane;
        const bool in = i < E.n;
        bool valid = true;
        int64_t val = 0;
        if (in) {
            int64_t pid = E.ids[i] >> 32, gid = E.ids[i] & 0xffffffffLL;
            int64_t ps = E.pstart[pid - 1], pe = E.pstart[pid] - 1;
            int64_t e = E.frame == AMD_WFN_FRAME_ROWS ? i
                        : E.frame == AMD_WFN_FRAME_RANGE
                            ? E.gstart[gid] - 1 : pe;
            switch (E.fn) {
            case AMD_WFN_RANK:
                val = E.gstart[gid - 1] - ps + 1;
                break;
            case AMD_WFN_DENSE_RANK:
                val = gid - (E.ids[ps] & 0xffffffffLL) + 1;
                break;
            case AMD_WFN_LAG:
            case AMD_WFN_LEAD: {
                bool lag = E.fn == AMD_WFN_LAG;
                if (E.k <= (lag ? i - ps : pe - i))
                    val = E.arg[E.perm[lag ? i - E.k : i + E.k]];
                else if (E.has_default)
                    val = E.default_value;
                else
                    valid = false;
                break;
            }
            case AMD_WFN_FIRST_VALUE:
                val = E.arg[E.perm[ps]];
                break;
            case AMD_WFN_LAST_VALUE:
                val = E.arg[E.perm[e]];
                break;
            case AMD_WFN_COUNT:
                val = e - ps + 1;
                break;
            default:   /* SUM MIN MAX */
                val = E.scan[e];
            }
        }
        if (E.vbits) {
            unsigned long long bits = __ballot(in && valid);
            if (lane == 0) E.vbits[wbase >> 6] = bits;
        }
        if (!in || (E.limit && val > E.limit)) continue;
        int64_t r = E.limit ? (int64_t)atomicAdd(E.n_out, 1ULL) : E.base + i;
        if (r >= E.out_cap) { *E.err = WERR_OUT_CAP; continue; }
        for (int c = 0; c < E.n_data; c++)
            E.out[c][r] = E.scratch[(size_t)c * E.scap + E.perm[i]];
        E.out[E.n_data][r] = (int64_t)E.instant;
        E.out[E.n_data + 1][r] = val;
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
    /* cfg.fn != ROW_NUMBER only */
    int64_t *gstart;          /* peer-group starts; segstart = partitions' */
    int64_t *scan;            /* SUM MIN MAX */
    int *scan_pf;
    int64_t *scan_pv;
    unsigned long long *vbits;   /* validity words of one watermark's output */
    int64_t vbits_cap;
    /* limit == 0: where each fired instant's rows went, known on the host */
    struct Fired { int64_t base, n, word; };
    std::vector<Fired> fired;
    int64_t emit_base, emit_word;
};

static bool wfn_takes_arg(int fn) {
    return fn == AMD_WFN_LAG || fn == AMD_WFN_LEAD ||
           fn == AMD_WFN_FIRST_VALUE || fn == AMD_WFN_LAST_VALUE ||
           fn == AMD_WFN_SUM || fn == AMD_WFN_MIN || fn == AMD_WFN_MAX;
}

static bool wfn_has_frame(int fn) {
    return fn >= AMD_WFN_FIRST_VALUE && fn <= AMD_WFN_MAX;
}

/* the appended fields; nullptr = fine, else the one message of the cause */
static const char *wfn_check(const AmdWindowFnConfig *c, char *buf,
                             size_t len) {
    const int fn = c->fn;
    if (fn < AMD_WFN_ROW_NUMBER || fn > AMD_WFN_MAX) {
        snprintf(buf, len, "unknown window function %d", fn);
    } else if (c->frame < AMD_WFN_FRAME_RANGE ||
               c->frame > AMD_WFN_FRAME_PARTITION) {
        snprintf(buf, len, "unknown window frame %d", c->frame);
    } else if ((wfn_takes_arg(fn) ||
                (fn == AMD_WFN_COUNT && c->arg_col != -1)) &&
               (c->arg_col < 0 || c->arg_col > c->n_cols - 2)) {
        snprintf(buf, len,
                 "arg_col %d out of range [0, %d] for a window function "
                 "with an argument", c->arg_col, c->n_cols - 2);
    } else if ((fn == AMD_WFN_RANK || fn == AMD_WFN_DENSE_RANK) ?
                   c->arg_col != -1
                   : fn == AMD_WFN_ROW_NUMBER && c->arg_col != -1 &&
                         c->arg_col != 0) {
        snprintf(buf, len,
                 "arg_col must be -1 for a window function without an "
                 "argument, got %d", c->arg_col);
    } else if (c->offset < 0) {
        snprintf(buf, len, "LAG/LEAD offset must be >= 0, got %lld",
                 (long long)c->offset);
    } else if (c->limit != 0 && fn != AMD_WFN_ROW_NUMBER &&
               fn != AMD_WFN_RANK && fn != AMD_WFN_DENSE_RANK) {
        snprintf(buf, len,
                 "limit is only for ROW_NUMBER, RANK and DENSE_RANK");
    } else if (c->frame != AMD_WFN_FRAME_RANGE && !wfn_has_frame(fn)) {
        snprintf(buf, len,
                 "frame must be 0 for ROW_NUMBER, the rank functions and "
                 "LAG/LEAD, which ignore frames");
    } else {
        return nullptr;
    }
    return buf;
}

API void *arroyo_amd_windowfn_create(const AmdWindowFnConfig *cfg) {
    if (!cfg || cfg->n_cols < 2 || cfg->n_cols > 12 || cfg->n_order < 1 ||
        cfg->n_order > 2 || cfg->part_col >= cfg->n_cols - 1) {
        snprintf(g_create_err, sizeof g_create_err, "invalid windowfn config");
        return nullptr;
    }
    if (wfn_check(cfg, g_create_err, sizeof g_create_err)) return nullptr;
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
    /* k_wf_starts writes one entry past the last partition */
    OP_ALLOC(o, o->segstart,
             (plane + (cfg->fn != AMD_WFN_ROW_NUMBER ? 1 : 0)) * 8);
    if (cfg->fn != AMD_WFN_ROW_NUMBER) {
        size_t tiles = plane / AMD_WFN_SCAN_TILE + 1;
        OP_ALLOC(o, o->gstart, (plane + 1) * 8);
        if (cfg->fn == AMD_WFN_SUM || cfg->fn == AMD_WFN_MIN ||
            cfg->fn == AMD_WFN_MAX) {
            OP_ALLOC(o, o->scan, plane * 8);
            OP_ALLOC(o, o->scan_pf, tiles * 4);
            OP_ALLOC(o, o->scan_pv, tiles * 8);
        }
        if ((cfg->fn == AMD_WFN_LAG || cfg->fn == AMD_WFN_LEAD) &&
            !cfg->has_default) {
            /* every fired instant starts a new word */
            o->vbits_cap = o->out_cap / 64 + o->I + 1;
            OP_ALLOC(o, o->vbits, (size_t)o->vbits_cap * 8);
        }
    }
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

/* retire a fired group's slots */
static int wf_retire(GpuWindowFn *o, const std::vector<uint32_t> &slots) {
    for (uint32_t s : slots) {
        HIP_CHECK(o, hipMemsetAsync(o->tag + s, 0xFF, 8, o->stream));
        HIP_CHECK(o, hipMemsetAsync(o->cursor + s, 0, 8, o->stream));
    }
    return 0;
}

template <int OP>
static int wf_scan(GpuWindowFn *o, const WfScanArgs &S) {
    hipLaunchKernelGGL(k_wf_scan_reduce<OP>, dim3((unsigned)S.n_tiles),
                       dim3(256), 0, o->stream, S);
    HIP_CHECK(o, hipGetLastError());
    hipLaunchKernelGGL(k_wf_scan_partials<OP>, dim3(1), dim3(256), 0,
                       o->stream, S);
    HIP_CHECK(o, hipGetLastError());
    hipLaunchKernelGGL(k_wf_scan_down<OP>, dim3((unsigned)S.n_tiles),
                       dim3(256), 0, o->stream, S);
    HIP_CHECK(o, hipGetLastError());
    return 0;
}

/* cfg.fn != ROW_NUMBER: everything after the sort of one instant's n rows */
static int wf_fire_fn(GpuWindowFn *o, uint64_t instant, int64_t n) {
    const AmdWindowFnConfig &c = o->cfg;
    auto col = [&](int i) { return o->scratch + (size_t)i * o->scap; };
    hipLaunchKernelGGL(k_wf_flags, dim3(grid_for(n, 2048)), dim3(256), 0,
                       o->stream,
                       c.part_col >= 0 ? col(c.part_col) : nullptr,
                       col(c.order_col[0]),
                       c.n_order > 1 ? col(c.order_col[1]) : nullptr,
                       o->perm, o->hf, n);
    HIP_CHECK(o, hipGetLastError());
    size_t tmp = o->cub_bytes;
    HIP_CHECK(o, hipcub::DeviceScan::InclusiveSum(o->cub_tmp, tmp, o->hf,
                                                  o->segid, (int)n,
                                                  o->stream));
    hipLaunchKernelGGL(k_wf_starts, dim3(grid_for(n, 2048)), dim3(256), 0,
                       o->stream, o->hf, o->segid, o->segstart, o->gstart, n);
    HIP_CHECK(o, hipGetLastError());
    if (o->scan) {
        WfScanArgs S = {};
        S.arg = col(c.arg_col);
        S.perm = o->perm;
        S.hf = o->hf;
        S.n = n;
        S.n_tiles = (n + AMD_WFN_SCAN_TILE - 1) / AMD_WFN_SCAN_TILE;
        S.pf = o->scan_pf;
        S.pv = o->scan_pv;
        S.out = o->scan;
        if (c.fn == AMD_WFN_SUM ? wf_scan<SOP_ADD>(o, S)
            : c.fn == AMD_WFN_MIN ? wf_scan<SOP_MIN>(o, S)
                                  : wf_scan<SOP_MAX>(o, S))
            return 1;
    }
    WfFnArgs E = {};
    E.scratch = o->scratch;
    E.scap = o->scap;
    E.perm = o->perm;
    E.ids = o->segid;
    E.pstart = o->segstart;
    E.gstart = o->gstart;
    E.scan = o->scan;
    E.arg = c.arg_col >= 0 ? col(c.arg_col) : nullptr;
    E.n = n;
    E.n_data = o->n_data;
    E.fn = c.fn;
    E.frame = c.frame;
    E.k = c.offset;
    E.has_default = c.has_default;
    E.default_value = c.default_value;
    E.limit = c.limit;
    E.instant = instant;
    for (int i = 0; i < o->out_cols; i++) E.out[i] = o->d_out[i];
    E.n_out = o->d_n_out;
    E.out_cap = o->out_cap;
    E.err = o->d_err;
    if (!c.limit) {
        /* the rows land at base + sorted position: no cursor, and the
         * output order is the sort order */
        if (o->emit_base + n > o->out_cap) {
            snprintf(o->err_msg, sizeof o->err_msg, "%s",
                     wf_err_msg(WERR_OUT_CAP));
            return 1;
        }
        E.base = o->emit_base;
        if (o->vbits) E.vbits = o->vbits + o->emit_word;
        o->fired.push_back({o->emit_base, n, o->emit_word});
        o->emit_base += n;
        o->emit_word += (n + 63) / 64;
    }
    hipLaunchKernelGGL(k_wf_emit_fn, dim3(grid_for(n, 2048)), dim3(256), 0,
                       o->stream, E);
    HIP_CHECK(o, hipGetLastError());
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
    if (n == 0) return wf_retire(o, slots);
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
    if (c.fn != AMD_WFN_ROW_NUMBER) {
        if (wf_fire_fn(o, instant, n)) return 1;
        return wf_retire(o, slots);
    }
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
    return wf_retire(o, slots);
}

/* LAG/LEAD without a default: join the fired instants' validity words,
 * each instant's starting at bit 0 of a word of its own, into the function
 * column's bitmap.  A batch without a NULL gets no validity table. */
static int wf_fill_validity(GpuWindowFn *o, AmdOutBatch *out) {
    std::vector<unsigned long long> words((size_t)o->emit_word);
    if (words.empty()) return 0;
    hipError_t e = hipMemcpyAsync(words.data(), o->vbits, words.size() * 8,
                                  hipMemcpyDeviceToHost, o->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(o->stream);
    if (e != hipSuccess) out_free_host(out);
    HIP_CHECK(o, e);
    int64_t ones = 0;   /* bits past an instant's rows are clear */
    for (unsigned long long w : words) ones += __builtin_popcountll(w);
    if (ones == out->n_rows) return 0;
    uint8_t *bm = out_alloc_validity(out)
                      ? nullptr : out_validity_col(out, out->n_cols - 1);
    if (!bm) {
        out_free_host(out);
        snprintf(o->err_msg, sizeof o->err_msg,
                 "%s: validity bitmap allocation failed", __func__);
        return 1;
    }
    for (const GpuWindowFn::Fired &f : o->fired)
        out_validity_append_bits(
            bm, f.base, (const uint8_t *)(words.data() + f.word), f.n);
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
    o->fired.clear();
    o->emit_base = o->emit_word = 0;
    for (auto &kv : fired)
        if (wf_fire(o, kv.first, kv.second, cnt)) return 1;
    unsigned long long n = 0;
    HIP_CHECK(o, hipMemcpyAsync(&n, o->d_n_out, 8, hipMemcpyDeviceToHost,
                                o->stream));
    HIP_CHECK(o, hipStreamSynchronize(o->stream));
    if (op_check_err(o, wf_err_msg)) return 1;
    /* a function without a limit places its rows from the host */
    if (o->cfg.fn != AMD_WFN_ROW_NUMBER && !o->cfg.limit)
        n = (unsigned long long)o->emit_base;
    if (out) {
        if (op_out_alloc(o, out, (int64_t)n, o->out_cols, __func__)) return 1;
        if (out_copy_cols(o, out, o->d_out, (int64_t)n)) return 1;
        if (o->vbits && wf_fill_validity(o, out)) return 1;
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
    std::vector<int64_t> seq((size_t)total);
    int64_t r = 0;
    for (uint32_t s = 0; s < o->I; s++) {
        if (tags[s] == EMPTY_TAG || cnt[s] == 0) continue;
        int64_t n = (int64_t)cnt[s];
        for (int cdx = 0; cdx < ncols; cdx++)   /* the last plane: arrival */
            HIP_CHECK(o, hipMemcpyAsync(
                    cdx < ncols - 1 ? (int64_t *)out->cols[cdx] + r
                                    : seq.data() + r,
                    o->planes + (size_t)cdx * plane + (size_t)s * o->cap,
                    (size_t)n * 8, hipMemcpyDeviceToHost, o->stream));
        HIP_CHECK(o, hipStreamSynchronize(o->stream));
        for (int64_t j = 0; j < n; j++)
            ((int64_t *)out->cols[ncols - 1])[r + j] = (int64_t)tags[s];
        r += n;
    }
    /* A slot holds its rows in the order the append kernel's waves took
     * their places, not in arrival order.  Hand the rows back by arrival
     * stamp, so that the fresh stamps a restore gives them keep every tie
     * among peers where it was: the functions that read a row's
     * neighbours (LAG, LEAD, a ROWS frame) depend on it. */
    std::vector<int64_t> idx((size_t)total), tmp((size_t)total);
    for (int64_t i = 0; i < total; i++) idx[i] = i;
    std::sort(idx.begin(), idx.end(),
              [&](int64_t a, int64_t b) { return seq[a] < seq[b]; });
    for (int cdx = 0; cdx < ncols; cdx++) {
        int64_t *col = (int64_t *)out->cols[cdx];
        for (int64_t i = 0; i < total; i++) tmp[i] = col[idx[i]];
        memcpy(col, tmp.data(), (size_t)total * 8);
    }
    return 0;
}

API void arroyo_amd_windowfn_destroy(void *h) {
    delete (GpuWindowFn *)h;   /* ~OpBase drains the stream first */
}
