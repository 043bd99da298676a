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
 */
#include <hipcub/hipcub.hpp>

#include "op_common.h"
#include "../../include/arroyo_amd_map_check.h"

namespace mapop {

#define MERR_DIV0     1
#define MERR_OVERFLOW 2       /* INT64_MIN / -1 */
#define MERR_CAST     3       /* F2I of NaN, +-inf or outside [-2^63, 2^63) */

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
 * on the error word: which one is reported is unspecified. */
__device__ inline void map_eval(const AmdMapConfig &c, int64_t *regs,
                                int *err) {
    for (int i = 0; i < c.n_prog; i++) {
        const AmdMapInstr &in = c.prog[i];
        int64_t a = regs[in.a], b = regs[in.b], v = 0;
        uint64_t ua = (uint64_t)a, ub = (uint64_t)b;
        double fa = __longlong_as_double(a), fb = __longlong_as_double(b);
        switch (in.op) {
        case AMD_MOP_CONST: v = in.imm; break;
        case AMD_MOP_ADD: v = (int64_t)(ua + ub); break;
        case AMD_MOP_SUB: v = (int64_t)(ua - ub); break;
        case AMD_MOP_MUL: v = (int64_t)(ua * ub); break;
        case AMD_MOP_DIV:
            if (b == 0) { *err = MERR_DIV0; return; }
            if (a == INT64_MIN && b == -1) { *err = MERR_OVERFLOW; return; }
            v = a / b;
            break;
        case AMD_MOP_MOD:
            if (b == 0) { *err = MERR_DIV0; return; }
            v = b == -1 ? 0 : a % b;
            break;
        case AMD_MOP_EQ: v = a == b; break;
        case AMD_MOP_NE: v = a != b; break;
        case AMD_MOP_LT: v = a < b; break;
        case AMD_MOP_LE: v = a <= b; break;
        case AMD_MOP_GT: v = a > b; break;
        case AMD_MOP_GE: v = a >= b; break;
        case AMD_MOP_AND: v = (a != 0) && (b != 0); break;
        case AMD_MOP_OR: v = (a != 0) || (b != 0); break;
        case AMD_MOP_NOT: v = a == 0; break;
        case AMD_MOP_I2F: v = __double_as_longlong((double)a); break;
        case AMD_MOP_F2I:
            /* 0x1p63 == 2^63; a NaN fails both compares */
            if (!(fa >= -0x1p63 && fa < 0x1p63)) { *err = MERR_CAST; return; }
            v = (int64_t)fa;
            break;
        case AMD_MOP_FADD: v = __double_as_longlong(fa + fb); break;
        case AMD_MOP_FSUB: v = __double_as_longlong(fa - fb); break;
        case AMD_MOP_FMUL: v = __double_as_longlong(fa * fb); break;
        case AMD_MOP_FDIV: v = __double_as_longlong(fa / fb); break;
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
        for (int i = 0; i < A.n_in; i++) regs[i] = A.cols[i][r];
        map_eval(A.cfg, regs, A.err);
        for (int i = 0; i < A.cfg.n_out; i++)
            A.vals[i][r] = regs[A.cfg.out_reg[i]];
        if (A.keep)
            A.keep[r] = regs[A.cfg.filter_reg] != 0;
    }
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
 * surviving rows. */
static int map_eval(GpuMap *o, const int64_t *const *dcols, int32_t n_cols,
                    int64_t n_rows, const int64_t **src, int64_t *n_keep) {
    const AmdMapConfig &c = o->cfg;
    MapArgs A = {};
    for (int cc = 0; cc < n_cols; cc++) A.cols[cc] = dcols[cc];
    A.n_in = n_cols;
    A.n_rows = n_rows;
    A.cfg = c;
    A.keep = c.filter_reg >= 0 ? o->d_keep : nullptr;
    for (int i = 0; i < c.n_out; i++) src[i] = A.vals[i] = o->d_vals[i];
    A.err = o->d_err;
    hipLaunchKernelGGL(k_map_eval, dim3(grid_for(n_rows, 2048)), dim3(256), 0,
                       o->stream, A);
    HIP_CHECK(o, hipGetLastError());
    *n_keep = n_rows;
    if (c.filter_reg >= 0 && n_rows > 0) {
        size_t tmp = o->cub_bytes;
        HIP_CHECK(o, hipcub::DeviceScan::ExclusiveSum(
                         o->cub_tmp, tmp, o->d_keep, o->d_pos, (int)n_rows,
                         o->stream));
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
    if (!op_check_err(o, map_err_msg)) return 0;
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

static int map_run(GpuMap *o, const int64_t *const *cols, int32_t n_cols,
                   int64_t n_rows, AmdOutBatch *out) {
    const AmdMapConfig &c = o->cfg;
    if (map_check_cols(o, n_cols)) return 1;
    /* room for every input row; n_rows is set to what survives */
    if (op_out_alloc(o, out, n_rows, c.n_out, __func__)) return 1;
    for (int i = 0; i < c.n_out; i++) out->is_f64[i] = c.out_is_f64[i];
    int64_t emitted = 0;
    int64_t done = 0;
    while (done < n_rows) {
        int64_t take = n_rows - done;
        if (take > o->cap) take = o->cap;
        const int64_t *dcols[AMD_MAP_MAX_REGS], *src[AMD_MAP_MAX_OUT];
        int64_t n_keep = 0;
        if (o->stg.stage_chunk(o, cols, n_cols, done, take, dcols) ||
            map_eval(o, dcols, n_cols, take, src, &n_keep))
            return 1;
        for (int i = 0; i < c.n_out && n_keep; i++)
            HIP_CHECK(o, hipMemcpyAsync((int64_t *)out->cols[i] + emitted,
                                        src[i], (size_t)n_keep * 8,
                                        hipMemcpyDeviceToHost, o->stream));
        /* staging and d_vals are reused by the next chunk */
        HIP_CHECK(o, hipStreamSynchronize(o->stream));
        emitted += n_keep;
        done += take;
    }
    out->n_rows = emitted;
    /* give back what the filter dropped; a shrinking realloc that fails
     * leaves the column as it was */
    size_t keep_bytes = (size_t)(emitted ? emitted : 1) * 8;
    for (int i = 0; i < c.n_out && emitted < n_rows; i++)
        if (void *p = realloc(out->cols[i], keep_bytes)) out->cols[i] = p;
    return 0;
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
    if (map_check_cols(o, n_cols)) return 1;
    if (n_rows > o->cap) {
        snprintf(o->err_msg, sizeof o->err_msg,
                 "device batch of %lld rows exceeds capacity %lld",
                 (long long)n_rows, (long long)o->cap);
        return 1;
    }
    return map_eval(o, dcols, n_cols, n_rows, d_out_cols, n_out_rows);
}

API int arroyo_amd_map_process_batch(void *h, const int64_t *const *cols,
                                     int32_t n_cols, int64_t n_rows,
                                     AmdOutBatch *out) {
    GpuMap *o = (GpuMap *)h;
    memset(out, 0, sizeof *out); /* so early-validation errors leave a
                                  * well-defined (empty) out */
    int rc = map_run(o, cols, n_cols, n_rows, out);
    /* error exits (device error, HIP failure) must not leak the partially
     * filled output the caller will never free */
    if (rc) out_free_host(out);
    return rc;
}

API void arroyo_amd_map_destroy(void *h) {
    delete (GpuMap *)h;   /* ~OpBase drains the stream first */
}
