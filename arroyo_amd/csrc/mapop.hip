/* arroyo-amd stateless map/filter/projection: MI355X-native (gfx950)
 * equivalent of ValueExecutionOperator / ProjectionOperator /
 * KeyExecutionOperator (crates/arroyo-worker/src/arrow/mod.rs:48-243)
 * behind the arroyo_amd_map_* C ABI (include/arroyo_amd.h).
 *
 * The reference evaluates a serialized DataFusion expression plan per batch
 * (StatelessPhysicalExecutor :245-290).  Here the plan's information
 * content is a register program (AmdMapConfig) interpreted by one fused
 * kernel: registers live in VGPRs, the instruction stream is wave-uniform
 * (no divergence beyond the filter), and the whole op is a bandwidth-bound
 * streaming map.  Filtered output preserves row order exactly like the
 * reference's filter kernels: keep flags -> hipCUB exclusive scan ->
 * ordered scatter, three launches per batch on one stream.
 *
 * Parity is pinned against oracle/arroyo_oracle.c by tests/test_mapop.py
 * (bit-exact, including the f64 bit patterns); every opcode's semantics,
 * the launch shapes and the device surface are pinned against an
 * independent reference by tests/test_mapop_ops.py.
 *
 * SQL NULLs (AmdMapConfig.null_semantics = 1, rules in
 * include/arroyo_amd_types.h; restated from arrow-arith / DataFusion, not
 * golden-pinned, checked by tests/test_mapop_null.py).  A null_semantics = 0
 * handle launches k_map_eval / k_map_scatter exactly as before.  A nullable
 * handle launches k_map_eval_nullable: each row carries one uint32_t of
 * validity, bit r for register r, evaluated next to the values.  A wave's 64
 * consecutive rows are one aligned 64-bit word of every Arrow bitmap, so an
 * input bitmap costs one wave-uniform load per wave and column, and an
 * unfiltered output bitmap is one __ballot per column and one 8-byte store
 * by lane 0.  Under a filter the rows move, so validity travels through the
 * ordered compaction as one mask byte per row (bit i = output column i;
 * n_out <= 6 here): k_map_scatter_nullable moves the byte with the row and
 * k_map_pack_validity ballots the compacted bytes into bitmaps.  No atomics
 * touch a bitmap, so the bytes are the same on every run; the per-column
 * NULL counts are popcounts of those ballots, summed per block and added
 * with one integer atomicAdd per block, and ride the end-of-batch readback.
 */
#include <hipcub/hipcub.hpp>

#include "op_common.h"
#define AMD_MAP_CHECK_NULLABLE
#include "../../include/arroyo_amd_map_check.h"

namespace mapop {

#define MERR_DIV0     1
#define MERR_OVERFLOW 2       /* INT64_MIN / -1 */
#define MERR_CAST     3       /* F2I of NaN, +-inf or outside [-2^63, 2^63) */

#define MAP_GPU_MAX_OUT 6     /* the scatter kernels take six columns */

struct MapArgs {
    const int64_t *cols[AMD_MAP_MAX_REGS];
    int32_t n_in;
    int64_t n_rows;
    AmdMapConfig cfg;          /* program in kernel args (constant memory) */
    int64_t *keep;             /* [n] 0/1 (filter) */
    int64_t *vals[AMD_MAP_MAX_OUT]; /* unfiltered per-row results */
    int *err;
};

/* Row arithmetic, restated from arrow-arith / DataFusion (COVERAGE.md row
 * 3): + - * wrap (unsigned arithmetic: no signed-overflow UB); DIV
 * truncates, errors on b == 0 and on INT64_MIN / -1; MOD takes the
 * dividend's sign, errors on b == 0, and x % -1 == 0 for every x; compares
 * and AND/OR/NOT see the raw i64 and give exactly 0 or 1; F2I truncates and
 * errors on NaN, +-inf and anything outside [-2^63, 2^63); f64 ops are IEEE
 * binary64.  A row error stops that row's program; the call then fails and
 * the row's outputs are never read.  Rows that raise different errors race
 * on the error word: which one is reported is unspecified.
 *
 * NS (null_semantics = 1): bit r of `valid` says register r is non-NULL.
 * `ok` is the validity of the instruction's result; a NULL result stores 0
 * and raises no error, and a NULL register always holds 0, so the value
 * under a NULL never reaches a result.  With NS = false every `NS` branch
 * folds away and this is the plain machine. */
template <bool NS>
__device__ inline void map_eval(const AmdMapConfig &c, int64_t *regs,
                                uint32_t &valid, int *err) {
    for (int i = 0; i < c.n_prog; i++) {
        const AmdMapInstr &in = c.prog[i];
        int64_t a = regs[in.a], b = regs[in.b], v = 0;
        uint64_t ua = (uint64_t)a, ub = (uint64_t)b;
        double fa = __longlong_as_double(a), fb = __longlong_as_double(b);
        bool va = true, vb = true, ok = true;
        if (NS) {
            va = valid >> in.a & 1u;
            vb = valid >> in.b & 1u;
            if (in.op > AMD_MOP_FDIV) {
                switch (in.op) {
                case AMD_MOP_IS_NULL: v = !va; break;
                case AMD_MOP_IS_NOT_NULL: v = va; break;
                case AMD_MOP_COALESCE:
                    v = va ? a : b;
                    ok = va || vb;
                    break;
                case AMD_MOP_NULLIF:
                    v = a;
                    ok = va && !(vb && a == b);
                    break;
                case AMD_MOP_SELECT: {
                    int e = (int)in.imm & (AMD_MAP_MAX_REGS - 1);
                    bool cond = va && a != 0;
                    v = cond ? b : regs[e];
                    ok = cond ? vb : (bool)(valid >> e & 1u);
                    break;
                }
                }
                regs[in.dst] = ok ? v : 0;
                valid = (valid & ~(1u << in.dst)) | ((uint32_t)ok << in.dst);
                continue;
            }
            /* propagation: NULL if any operand the op reads is NULL
             * (AND / OR refine it below) */
            bool unary = in.op == AMD_MOP_NOT || in.op == AMD_MOP_I2F ||
                         in.op == AMD_MOP_F2I;
            ok = in.op == AMD_MOP_CONST || (va && (unary || vb));
        }
        switch (in.op) {
        case AMD_MOP_CONST: v = in.imm; break;
        case AMD_MOP_ADD: v = (int64_t)(ua + ub); break;
        case AMD_MOP_SUB: v = (int64_t)(ua - ub); break;
        case AMD_MOP_MUL: v = (int64_t)(ua * ub); break;
        case AMD_MOP_DIV:
            if (NS && !ok) break;       /* NULL result: no error */
            if (b == 0) { *err = MERR_DIV0; return; }
            if (a == INT64_MIN && b == -1) { *err = MERR_OVERFLOW; return; }
            v = a / b;
            break;
        case AMD_MOP_MOD:
            if (NS && !ok) break;
            if (b == 0) { *err = MERR_DIV0; return; }
            v = b == -1 ? 0 : a % b;
            break;
        case AMD_MOP_EQ: v = a == b; break;
        case AMD_MOP_NE: v = a != b; break;
        case AMD_MOP_LT: v = a < b; break;
        case AMD_MOP_LE: v = a <= b; break;
        case AMD_MOP_GT: v = a > b; break;
        case AMD_MOP_GE: v = a >= b; break;
        case AMD_MOP_AND:
            v = (a != 0) && (b != 0);
            /* Kleene: a valid false decides, else a NULL side is NULL */
            if (NS) ok = (va && a == 0) || (vb && b == 0) || (va && vb);
            break;
        case AMD_MOP_OR:
            v = (a != 0) || (b != 0);
            if (NS) ok = (va && a != 0) || (vb && b != 0) || (va && vb);
            break;
        case AMD_MOP_NOT: v = a == 0; break;
        case AMD_MOP_I2F: v = __double_as_longlong((double)a); break;
        case AMD_MOP_F2I:
            if (NS && !ok) break;
            /* 0x1p63 == 2^63; a NaN fails both compares */
            if (!(fa >= -0x1p63 && fa < 0x1p63)) { *err = MERR_CAST; return; }
            v = (int64_t)fa;
            break;
        case AMD_MOP_FADD: v = __double_as_longlong(fa + fb); break;
        case AMD_MOP_FSUB: v = __double_as_longlong(fa - fb); break;
        case AMD_MOP_FMUL: v = __double_as_longlong(fa * fb); break;
        case AMD_MOP_FDIV: v = __double_as_longlong(fa / fb); break;
        }
        if (NS) {
            if (!ok) v = 0;
            valid = (valid & ~(1u << in.dst)) | ((uint32_t)ok << in.dst);
        }
        regs[in.dst] = v;
    }
}

__global__ void __launch_bounds__(256)
k_map_eval(MapArgs A) {
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         r < A.n_rows; r += stride) {
        int64_t regs[AMD_MAP_MAX_REGS];
        uint32_t all_valid = 0;    /* unused by the plain machine */
        for (int i = 0; i < A.n_in; i++) regs[i] = A.cols[i][r];
        map_eval<false>(A.cfg, regs, all_valid, A.err);
        for (int i = 0; i < A.cfg.n_out; i++)
            A.vals[i][r] = regs[A.cfg.out_reg[i]];
        if (A.keep)
            A.keep[r] = regs[A.cfg.filter_reg] != 0;
    }
}

/* the nullable machine's extra arguments */
struct MapArgsN {
    MapArgs A;
    const uint64_t *valid[AMD_MAP_MAX_REGS]; /* input bitmaps as 64-bit
                                              * words; null = all valid */
    uint64_t *obm[MAP_GPU_MAX_OUT]; /* no filter: output bitmaps */
    uint8_t *ovm;                   /* filter: [n] output validity per row,
                                     * bit i = output column i */
    unsigned long long *nullc;      /* no filter: NULLs per output column */
};

/* NULL counts of a block: lane 0 of each wave keeps its popcounts in
 * registers across the grid-stride loop, the block adds them up in LDS, and
 * one global atomicAdd per block and column follows (one per wave and word
 * queued every wave of the grid on a single address: it doubled the batch
 * time at 10% NULLs).  Called once, by every thread of the block. */
__device__ inline void map_add_null_counts(const int *mine, int n_out,
                                           unsigned long long *nullc) {
    __shared__ unsigned int s_nulls[MAP_GPU_MAX_OUT];
    if (threadIdx.x < MAP_GPU_MAX_OUT) s_nulls[threadIdx.x] = 0;
    __syncthreads();
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int i = 0; i < MAP_GPU_MAX_OUT; i++)
            if (mine[i]) atomicAdd(&s_nulls[i], (unsigned int)mine[i]);
    __syncthreads();
    if ((int)threadIdx.x < n_out && s_nulls[threadIdx.x])
        atomicAdd(&nullc[threadIdx.x],
                  (unsigned long long)s_nulls[threadIdx.x]);
}

/* Wave `w` of the grid owns rows [64 w, 64 w + 64): word w of every bitmap.
 * The word index is wave-uniform (readfirstlane), so the trip count is too
 * and every lane reaches every __ballot; lanes past n_rows vote 0, which
 * leaves the padding bits of the last word clear.  The stride is a whole
 * number of waves. */
__global__ void __launch_bounds__(256)
k_map_eval_nullable(MapArgsN N) {
    const MapArgs &A = N.A;
    int lane = (int)(threadIdx.x & 63);
    int wave = __builtin_amdgcn_readfirstlane(
        (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    int n_waves = (int)((gridDim.x * blockDim.x) >> 6);
    int nulls[MAP_GPU_MAX_OUT] = {};   /* lane 0's, per output column */
    for (int64_t w = wave; w * 64 < A.n_rows; w += n_waves) {
        int64_t r = w * 64 + lane;
        bool in = r < A.n_rows;
        int64_t regs[AMD_MAP_MAX_REGS];
        uint32_t valid = 0;
        for (int i = 0; i < A.n_in; i++) {
            uint64_t word = N.valid[i] ? N.valid[i][w] : ~0ULL;
            bool ok = in && (word >> lane & 1ULL);
            /* whatever lies under a NULL is never loaded into the machine */
            regs[i] = ok ? A.cols[i][r] : 0;
            valid |= (uint32_t)ok << i;
        }
        if (in) map_eval<true>(A.cfg, regs, valid, A.err);
        unsigned long long full = __ballot(in);
        uint32_t om = 0;
#pragma unroll
        for (int i = 0; i < MAP_GPU_MAX_OUT; i++) {
            if (i >= A.cfg.n_out) break;
            int reg = A.cfg.out_reg[i];
            bool ok = in && (valid >> reg & 1u);
            if (in) A.vals[i][r] = ok ? regs[reg] : 0;
            om |= (uint32_t)ok << i;
            if (A.keep) continue;
            unsigned long long bits = __ballot(ok);
            if (lane == 0) N.obm[i][w] = bits;
            nulls[i] += __popcll(full & ~bits);
        }
        if (A.keep && in) {
            int f = A.cfg.filter_reg;
            /* a NULL predicate drops the row */
            A.keep[r] = (valid >> f & 1u) && regs[f] != 0;
            N.ovm[r] = (uint8_t)om;
        }
    }
    /* under a filter the counts come from k_map_pack_validity */
    if (!A.keep) map_add_null_counts(nulls, A.cfg.n_out, N.nullc);
}

/* ordered scatter of kept rows: pos = exclusive scan of keep flags */
__global__ void __launch_bounds__(256)
k_map_scatter(const int64_t *keep, const int64_t *pos,
              const int64_t *const vals0, const int64_t *const vals1,
              const int64_t *const vals2, const int64_t *const vals3,
              const int64_t *const vals4, const int64_t *const vals5,
              int64_t *out0, int64_t *out1, int64_t *out2, int64_t *out3,
              int64_t *out4, int64_t *out5, int n_out, int64_t n) {
    const int64_t *vals[6] = {vals0, vals1, vals2, vals3, vals4, vals5};
    int64_t *outs[6] = {out0, out1, out2, out3, out4, out5};
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         r < n; r += stride) {
        if (!keep[r]) continue;
        int64_t p = pos[r];
        for (int i = 0; i < n_out; i++) outs[i][p] = vals[i][r];
    }
}

/* the same scatter, the row's validity byte moving with it */
struct ScatterArgsN {
    const int64_t *keep, *pos;
    const int64_t *vals[MAP_GPU_MAX_OUT];
    int64_t *out[MAP_GPU_MAX_OUT];
    const uint8_t *ovm;        /* [n] per input row */
    uint8_t *omask;            /* [n_keep] per kept row */
    int32_t n_out;
    int64_t n;
};

__global__ void __launch_bounds__(256)
k_map_scatter_nullable(ScatterArgsN S) {
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         r < S.n; r += stride) {
        if (!S.keep[r]) continue;
        int64_t p = S.pos[r];
        for (int i = 0; i < S.n_out; i++) S.out[i][p] = S.vals[i][r];
        S.omask[p] = S.ovm[r];
    }
}

/* Compacted validity bytes -> one Arrow bitmap per output column, and the
 * NULL count of each from the popcounts.  The kept count is still on the
 * device (pos[last] + keep[last]), so this runs before the batch's one
 * readback; n > 0.  Same wave-per-word walk as k_map_eval_nullable. */
struct PackArgsN {
    const uint8_t *omask;
    const int64_t *keep, *pos;
    int64_t n;                 /* input rows of the batch */
    int32_t n_out;
    uint64_t *bm[MAP_GPU_MAX_OUT];
    unsigned long long *nullc;
};

__global__ void __launch_bounds__(256)
k_map_pack_validity(PackArgsN P) {
    int64_t n_keep = P.pos[P.n - 1] + P.keep[P.n - 1];
    int lane = (int)(threadIdx.x & 63);
    int wave = __builtin_amdgcn_readfirstlane(
        (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    int n_waves = (int)((gridDim.x * blockDim.x) >> 6);
    int nulls[MAP_GPU_MAX_OUT] = {};
    for (int64_t w = wave; w * 64 < n_keep; w += n_waves) {
        int64_t r = w * 64 + lane;
        bool in = r < n_keep;
        uint32_t m = in ? P.omask[r] : 0u;
        unsigned long long full = __ballot(in);
#pragma unroll
        for (int i = 0; i < MAP_GPU_MAX_OUT; i++) {
            if (i >= P.n_out) break;
            unsigned long long bits = __ballot(m >> i & 1u);
            if (lane == 0) P.bm[i][w] = bits;
            nulls[i] += __popcll(full & ~bits);
        }
    }
    map_add_null_counts(nulls, P.n_out, P.nullc);
}

}  // namespace mapop

using namespace mapop;


struct GpuMap : OpBase {
    AmdMapConfig cfg;
    int64_t cap;               /* per-batch row capacity */
    int64_t *d_vals[AMD_MAP_MAX_OUT];
    int64_t *d_out[AMD_MAP_MAX_OUT];
    int64_t *d_keep, *d_pos;
    void *cub_tmp;
    size_t cub_bytes;
    Staging stg;
    /* null_semantics = 1 only (null pointers otherwise); bitmaps are
     * bm_words 64-bit words, the capacity's worth */
    int64_t bm_words;
    uint64_t *d_obm[MAP_GPU_MAX_OUT];   /* output bitmaps */
    uint64_t *h_obm[MAP_GPU_MAX_OUT];   /* pinned: their host landing */
    uint8_t *d_ovm, *d_omask;           /* validity byte per row, before
                                         * and after the compaction */
    unsigned long long *d_nullc;        /* [MAP_GPU_MAX_OUT] */
    Staging stg_v;                      /* input bitmap staging */
};

API void *arroyo_amd_map_create(const AmdMapConfig *cfg) {
    /* k_map_scatter takes its columns as six kernel arguments */
    const char *bad = amd_map_config_error(cfg, AMD_MAP_MAX_OUT);
    if (!bad && cfg->n_out > 6)
        bad = "invalid map config: n_out <= 6 on the GPU path";
    if (bad) {
        snprintf(g_create_err, sizeof g_create_err, "%s", bad);
        return nullptr;
    }
    GpuMap *o = new GpuMap();
    o->cfg = *cfg;
    o->cap = 1 << 20;
    if (hipSetDevice(cfg->device) != hipSuccess) {
        snprintf(g_create_err, sizeof g_create_err,
                 "hipSetDevice(%d) failed: no HIP device (no CPU fallback)",
                 cfg->device);
        delete o;
        return nullptr;
    }
    for (int i = 0; i < cfg->n_out; i++) {
        OP_TRY(o, "map alloc", o->dev_alloc(o->d_vals[i], (size_t)o->cap * 8));
        OP_TRY(o, "map alloc", o->dev_alloc(o->d_out[i], (size_t)o->cap * 8));
    }
    OP_TRY(o, "map alloc", o->dev_alloc(o->d_keep, (size_t)o->cap * 8));
    OP_TRY(o, "map alloc", o->dev_alloc(o->d_pos, (size_t)o->cap * 8));
    OP_TRY(o, "map alloc", o->dev_alloc(o->d_err, 4, 0));
    OP_TRY(o, "map alloc", o->stg.alloc(o, cfg->n_in_cols, o->cap));
    if (cfg->null_semantics) {
        o->bm_words = (o->cap + 63) / 64;
        size_t bm_bytes = (size_t)o->bm_words * 8;
        for (int i = 0; i < cfg->n_out; i++) {
            OP_TRY(o, "map alloc", o->dev_alloc(o->d_obm[i], bm_bytes));
            OP_TRY(o, "map alloc", o->pinned_alloc(o->h_obm[i], bm_bytes));
        }
        OP_TRY(o, "map alloc", o->dev_alloc(o->d_ovm, (size_t)o->cap));
        OP_TRY(o, "map alloc", o->dev_alloc(o->d_omask, (size_t)o->cap));
        OP_TRY(o, "map alloc",
               o->dev_alloc(o->d_nullc, MAP_GPU_MAX_OUT * 8, 0));
        OP_TRY(o, "map alloc",
               o->stg_v.alloc(o, cfg->n_in_cols, o->bm_words));
    }
    o->cub_bytes = 0;
    OP_TRY(o, "map cub size",
           hipcub::DeviceScan::ExclusiveSum(nullptr, o->cub_bytes, o->d_keep,
                                            o->d_pos, (int)o->cap));
    OP_TRY_MSG(o, "map cub alloc failed",
               o->dev_alloc(o->cub_tmp, o->cub_bytes ? o->cub_bytes : 1));
    OP_TRY(o, "hipStreamCreate", o->stream_create(&o->stream));
    return o;
}

API const char *arroyo_amd_map_last_error(void *h) {
    return h ? ((GpuMap *)h)->err_msg : g_create_err;
}

static const char *map_err_msg(int e) {
    switch (e) {
    case MERR_DIV0: return "division by zero";
    case MERR_OVERFLOW: return "integer overflow in division";
    case MERR_CAST: return "cast of f64 to i64 out of range";
    }
    return "unknown map error";
}

/* evaluate the program over n_rows device rows, compact by the filter and
 * read the error word.  src[i] = where output column i landed, *n_keep =
 * surviving rows.
 *
 * A null_semantics = 1 handle takes dvalid (null, or per input column null
 * or its device bitmap as 64-bit words) and leaves output column i's bitmap
 * in d_obm[i] and its NULL count in null_counts[i]; the counts are read
 * back with the kept count (filter) or ahead of the error word (no filter),
 * under the synchronisation those already have. */
static int map_eval(GpuMap *o, const int64_t *const *dcols,
                    const uint64_t *const *dvalid, int32_t n_cols,
                    int64_t n_rows, const int64_t **src, int64_t *n_keep,
                    int64_t *null_counts) {
    const AmdMapConfig &c = o->cfg;
    const bool ns = c.null_semantics != 0;
    MapArgsN N = {};
    MapArgs &A = N.A;
    for (int cc = 0; cc < n_cols; cc++) A.cols[cc] = dcols[cc];
    A.n_in = n_cols;
    A.n_rows = n_rows;
    A.cfg = c;
    A.keep = c.filter_reg >= 0 ? o->d_keep : nullptr;
    for (int i = 0; i < c.n_out; i++) src[i] = A.vals[i] = o->d_vals[i];
    A.err = o->d_err;
    unsigned long long nullc[MAP_GPU_MAX_OUT] = {};
    if (ns) {
        for (int cc = 0; dvalid && cc < n_cols; cc++) N.valid[cc] = dvalid[cc];
        for (int i = 0; i < c.n_out; i++) N.obm[i] = o->d_obm[i];
        N.ovm = o->d_ovm;
        N.nullc = o->d_nullc;
        HIP_CHECK(o, hipMemsetAsync(o->d_nullc, 0, sizeof nullc, o->stream));
        hipLaunchKernelGGL(k_map_eval_nullable, dim3(grid_for(n_rows, 2048)),
                           dim3(256), 0, o->stream, N);
    } else {
        hipLaunchKernelGGL(k_map_eval, dim3(grid_for(n_rows, 2048)),
                           dim3(256), 0, o->stream, A);
    }
    HIP_CHECK(o, hipGetLastError());
    *n_keep = n_rows;
    if (c.filter_reg >= 0 && n_rows > 0) {
        size_t tmp = o->cub_bytes;
        HIP_CHECK(o, hipcub::DeviceScan::ExclusiveSum(
                         o->cub_tmp, tmp, o->d_keep, o->d_pos, (int)n_rows,
                         o->stream));
        if (ns) {
            ScatterArgsN S = {};
            PackArgsN P = {};
            S.keep = P.keep = o->d_keep;
            S.pos = P.pos = o->d_pos;
            for (int i = 0; i < c.n_out; i++) {
                S.vals[i] = o->d_vals[i];
                S.out[i] = o->d_out[i];
                P.bm[i] = o->d_obm[i];
            }
            S.ovm = o->d_ovm;
            S.omask = o->d_omask;
            P.omask = o->d_omask;
            S.n_out = P.n_out = c.n_out;
            S.n = P.n = n_rows;
            P.nullc = o->d_nullc;
            hipLaunchKernelGGL(k_map_scatter_nullable,
                               dim3(grid_for(n_rows, 2048)), dim3(256), 0,
                               o->stream, S);
            HIP_CHECK(o, hipGetLastError());
            hipLaunchKernelGGL(k_map_pack_validity,
                               dim3(grid_for(n_rows, 2048)), dim3(256), 0,
                               o->stream, P);
            HIP_CHECK(o, hipMemcpyAsync(nullc, o->d_nullc, sizeof nullc,
                                        hipMemcpyDeviceToHost, o->stream));
        } else {
            hipLaunchKernelGGL(
                k_map_scatter, dim3(grid_for(n_rows, 2048)), dim3(256), 0,
                o->stream, o->d_keep, o->d_pos, o->d_vals[0],
                c.n_out > 1 ? o->d_vals[1] : nullptr,
                c.n_out > 2 ? o->d_vals[2] : nullptr,
                c.n_out > 3 ? o->d_vals[3] : nullptr,
                c.n_out > 4 ? o->d_vals[4] : nullptr,
                c.n_out > 5 ? o->d_vals[5] : nullptr, o->d_out[0],
                c.n_out > 1 ? o->d_out[1] : nullptr,
                c.n_out > 2 ? o->d_out[2] : nullptr,
                c.n_out > 3 ? o->d_out[3] : nullptr,
                c.n_out > 4 ? o->d_out[4] : nullptr,
                c.n_out > 5 ? o->d_out[5] : nullptr, c.n_out, n_rows);
        }
        HIP_CHECK(o, hipGetLastError());
        /* n_keep = pos[last] + keep[last] */
        int64_t tail[2] = {0, 0};
        HIP_CHECK(o, hipMemcpyAsync(&tail[0], o->d_pos + (n_rows - 1), 8,
                                    hipMemcpyDeviceToHost, o->stream));
        HIP_CHECK(o, hipMemcpyAsync(&tail[1], o->d_keep + (n_rows - 1), 8,
                                    hipMemcpyDeviceToHost, o->stream));
        HIP_CHECK(o, hipStreamSynchronize(o->stream));
        *n_keep = tail[0] + tail[1];
    }
    if (c.filter_reg >= 0)
        for (int i = 0; i < c.n_out; i++) src[i] = o->d_out[i];
    else if (ns && n_rows > 0)   /* lands under op_check_err's sync */
        HIP_CHECK(o, hipMemcpyAsync(nullc, o->d_nullc, sizeof nullc,
                                    hipMemcpyDeviceToHost, o->stream));
    if (!op_check_err(o, map_err_msg)) {
        for (int i = 0; ns && i < c.n_out; i++)
            null_counts[i] = (int64_t)nullc[i];
        return 0;
    }
    /* reported once: clear the word so the next batch is judged afresh
     * (err_msg already holds this batch's message) */
    if (hipMemsetAsync(o->d_err, 0, 4, o->stream) == hipSuccess)
        (void)hipStreamSynchronize(o->stream);
    return 1;
}

static int map_check_cols(GpuMap *o, int32_t n_cols) {
    if (n_cols == o->cfg.n_in_cols) return 0;
    snprintf(o->err_msg, sizeof o->err_msg, "expected %d cols, got %d",
             o->cfg.n_in_cols, n_cols);
    return 1;
}

static int map_check_nullable(GpuMap *o) {
    if (o->cfg.null_semantics) return 0;
    snprintf(o->err_msg, sizeof o->err_msg,
             "nullable batch on a map handle created with "
             "null_semantics = 0");
    return 1;
}

/* host surface.  validity (null_semantics = 1 only): null, or per input
 * column null or its Arrow bitmap over all n_rows.  Chunks are `cap` = 2^20
 * rows, so a chunk's input bits start on a byte boundary; its kept count is
 * no multiple of 8 under a filter, so its output bits are appended at a bit
 * offset. */
static int map_run(GpuMap *o, const int64_t *const *cols,
                   const uint8_t *const *validity, int32_t n_cols,
                   int64_t n_rows, AmdOutBatch *out) {
    const AmdMapConfig &c = o->cfg;
    const bool ns = c.null_semantics != 0;
    if (map_check_cols(o, n_cols)) return 1;
    /* room for every input row; n_rows is set to what survives */
    if (op_out_alloc(o, out, n_rows, c.n_out, __func__)) return 1;
    for (int i = 0; i < c.n_out; i++) out->is_f64[i] = c.out_is_f64[i];
    if (ns) {
        bool ok = !out_alloc_validity(out);
        for (int i = 0; ok && i < c.n_out; i++)
            ok = out_validity_col(out, i) != nullptr;
        if (!ok) {
            snprintf(o->err_msg, sizeof o->err_msg,
                     "%s: validity bitmap allocation failed", __func__);
            return 1;
        }
    }
    int64_t nulls_total[MAP_GPU_MAX_OUT] = {};
    int64_t emitted = 0;
    int64_t done = 0;
    while (done < n_rows) {
        int64_t take = n_rows - done;
        if (take > o->cap) take = o->cap;
        const int64_t *dcols[AMD_MAP_MAX_REGS], *src[AMD_MAP_MAX_OUT];
        const uint64_t *dvalid[AMD_MAP_MAX_REGS] = {};
        int64_t nulls[MAP_GPU_MAX_OUT] = {};
        int64_t n_keep = 0;
        if (o->stg.stage_chunk(o, cols, n_cols, done, take, dcols)) return 1;
        for (int cc = 0; validity && cc < n_cols; cc++) {
            if (!validity[cc]) continue;
            size_t nbytes = (size_t)((take + 7) / 8);
            size_t nwords = (size_t)((take + 63) / 64);
            o->stg_v.h[cc][nwords - 1] = 0;   /* pad the last word */
            memcpy(o->stg_v.h[cc], validity[cc] + done / 8, nbytes);
            HIP_CHECK(o, hipMemcpyAsync(o->stg_v.d[cc], o->stg_v.h[cc],
                                        nwords * 8, hipMemcpyHostToDevice,
                                        o->stream));
            dvalid[cc] = (const uint64_t *)o->stg_v.d[cc];
        }
        if (map_eval(o, dcols, dvalid, n_cols, take, src, &n_keep, nulls))
            return 1;
        for (int i = 0; i < c.n_out && n_keep; i++)
            HIP_CHECK(o, hipMemcpyAsync((int64_t *)out->cols[i] + emitted,
                                        src[i], (size_t)n_keep * 8,
                                        hipMemcpyDeviceToHost, o->stream));
        /* only a bitmap with a NULL in it crosses to the host */
        for (int i = 0; ns && i < c.n_out; i++)
            if (nulls[i])
                HIP_CHECK(o, hipMemcpyAsync(o->h_obm[i], o->d_obm[i],
                                            (size_t)((n_keep + 63) / 64) * 8,
                                            hipMemcpyDeviceToHost,
                                            o->stream));
        /* staging and d_vals are reused by the next chunk */
        HIP_CHECK(o, hipStreamSynchronize(o->stream));
        for (int i = 0; ns && i < c.n_out; i++) {
            out_validity_append_bits(
                out->validity[i], emitted,
                nulls[i] ? (const uint8_t *)o->h_obm[i] : nullptr, n_keep);
            nulls_total[i] += nulls[i];
        }
        emitted += n_keep;
        done += take;
    }
    out->n_rows = emitted;
    /* give back what the filter dropped; a shrinking realloc that fails
     * leaves the column as it was */
    size_t keep_bytes = (size_t)(emitted ? emitted : 1) * 8;
    for (int i = 0; i < c.n_out && emitted < n_rows; i++)
        if (void *p = realloc(out->cols[i], keep_bytes)) out->cols[i] = p;
    if (ns) {
        /* an all-valid column has no bitmap, an all-valid batch no table */
        bool any = false;
        size_t bm_bytes = (size_t)((emitted + 7) / 8);
        for (int i = 0; i < c.n_out; i++) {
            if (!nulls_total[i]) {
                free(out->validity[i]);
                out->validity[i] = nullptr;
                continue;
            }
            any = true;
            if (void *p = realloc(out->validity[i], bm_bytes))
                out->validity[i] = (uint8_t *)p;
        }
        if (!any) {
            free(out->validity);
            out->validity = nullptr;
        }
    }
    return 0;
}

static int map_check_device_rows(GpuMap *o, int64_t n_rows) {
    if (n_rows <= o->cap) return 0;
    snprintf(o->err_msg, sizeof o->err_msg,
             "device batch of %lld rows exceeds capacity %lld",
             (long long)n_rows, (long long)o->cap);
    return 1;
}

/* device-resident map/filter: input columns already in HBM; output stays
 * in HBM.  Fills d_out_cols[i] with device addresses owned by the
 * operator (valid until the next process_batch* call) and *n_out_rows
 * with the surviving row count.  One launch, so n_rows must fit the
 * operator's chunk capacity (the host path chunks instead). */
API int arroyo_amd_map_process_batch_device(void *h,
                                            const int64_t *const *dcols,
                                            int32_t n_cols, int64_t n_rows,
                                            const int64_t **d_out_cols,
                                            int64_t *n_out_rows) {
    GpuMap *o = (GpuMap *)h;
    if (o->cfg.null_semantics) {
        snprintf(o->err_msg, sizeof o->err_msg,
                 "map_process_batch_device cannot return validity bitmaps: "
                 "a null_semantics = 1 handle takes "
                 "map_process_batch_nullable_device");
        return 1;
    }
    if (map_check_cols(o, n_cols) || map_check_device_rows(o, n_rows))
        return 1;
    return map_eval(o, dcols, nullptr, n_cols, n_rows, d_out_cols, n_out_rows,
                    nullptr);
}

/* the same with SQL NULLs: dvalidity is null, or per input column null (all
 * valid) or a device Arrow bitmap, 8-byte aligned and padded to a multiple
 * of 8 bytes, read in place as 64-bit words.  d_out_validity[i] is output
 * column i's device bitmap (operator-owned until the next call, 8-byte
 * aligned, padded to 8 bytes, padding bits clear) and null_counts[i], a host
 * value, its number of NULLs. */
API int arroyo_amd_map_process_batch_nullable_device(
    void *h, const int64_t *const *dcols, const uint8_t *const *dvalidity,
    int32_t n_cols, int64_t n_rows, const int64_t **d_out_cols,
    const uint8_t **d_out_validity, int64_t *null_counts,
    int64_t *n_out_rows) {
    GpuMap *o = (GpuMap *)h;
    if (map_check_nullable(o) || map_check_cols(o, n_cols) ||
        map_check_device_rows(o, n_rows))
        return 1;
    const uint64_t *dvalid[AMD_MAP_MAX_REGS] = {};
    for (int cc = 0; dvalidity && cc < n_cols; cc++) {
        if ((uintptr_t)dvalidity[cc] & 7) {
            snprintf(o->err_msg, sizeof o->err_msg,
                     "device validity bitmap of column %d is not 8-byte "
                     "aligned", cc);
            return 1;
        }
        dvalid[cc] = (const uint64_t *)dvalidity[cc];
    }
    if (map_eval(o, dcols, dvalid, n_cols, n_rows, d_out_cols, n_out_rows,
                 null_counts))
        return 1;
    for (int i = 0; i < o->cfg.n_out; i++)
        d_out_validity[i] = (const uint8_t *)o->d_obm[i];
    return 0;
}

static int map_process_host(GpuMap *o, const int64_t *const *cols,
                            const uint8_t *const *validity, int32_t n_cols,
                            int64_t n_rows, AmdOutBatch *out) {
    int rc = map_run(o, cols, validity, n_cols, n_rows, out);
    /* error exits (device error, HIP failure) must not leak the partially
     * filled output the caller will never free */
    if (rc) out_free_host(out);
    return rc;
}

/* on a null_semantics = 1 handle this means "every input valid"; the output
 * still carries bitmaps, since NULLIF and COALESCE make NULLs of their own */
API int arroyo_amd_map_process_batch(void *h, const int64_t *const *cols,
                                     int32_t n_cols, int64_t n_rows,
                                     AmdOutBatch *out) {
    memset(out, 0, sizeof *out); /* so early-validation errors leave a
                                  * well-defined (empty) out */
    return map_process_host((GpuMap *)h, cols, nullptr, n_cols, n_rows, out);
}

API int arroyo_amd_map_process_batch_nullable(
    void *h, const int64_t *const *cols, const uint8_t *const *validity,
    int32_t n_cols, int64_t n_rows, AmdOutBatch *out) {
    GpuMap *o = (GpuMap *)h;
    memset(out, 0, sizeof *out);
    if (map_check_nullable(o)) return 1;
    return map_process_host(o, cols, validity, n_cols, n_rows, out);
}

API void arroyo_amd_map_destroy(void *h) {
    delete (GpuMap *)h;   /* ~OpBase drains the stream first */
}

