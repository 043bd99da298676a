/* arroyo-amd updating (non-windowed) aggregate: MI355X-native (gfx950)
 * equivalent of IncrementalAggregatingFunc
 * (crates/arroyo-worker/src/arrow/incremental_aggregator.rs) behind the
 * arroyo_amd_updagg_* C ABI (include/arroyo_amd.h).
 *
 * MI355X-first design (NOT a translation of the reference's per-key
 * DataFusion Accumulator maps):
 *   - One device-resident open-addressing key table holds every key's
 *     retractable state: COUNT/SUM as signed atomicAdd words (retract =
 *     add of -1/-v, the reference's Sliding accumulators), AVG as
 *     (count, CAS-folded f64 sum), MIN/MAX as encoded atomicMax
 *     (append-only here; the reference re-aggregates a stored multiset),
 *     and COUNT DISTINCT as a per-(key, aggregate) chained value multiset
 *     in an append-only node pool (the reference's Batch accumulator,
 *     IncrementalState::Batch :84-174).  A value's net refcount may be
 *     split across duplicate chain nodes (two threads can race the first
 *     insert of the same value); the flush walk sums per value, so the
 *     count stays exact without any per-key locking.
 *   - MEDIAN / MIN_RETRACT / MAX_RETRACT (order statistics under
 *     retraction) keep the same chained multiset and are evaluated at flush
 *     by k_updagg_ordstat: one wavefront per changed (key, aggregate)
 *     gathers the chain's (value, net) nodes once into a per-wave LDS tile
 *     (or a global scratch arena when the chain is longer than the tile)
 *     and picks the wanted ranks with an MSB-first weighted radix select
 *     (up to 8 passes of 8 bits over a 256-bin LDS histogram of net
 *     counts; leading bytes shared by all of a key's values are skipped).
 *     Net counts are summed per bucket until the bucket is one value, so a
 *     value whose refcount is split into +k / -k nodes weighs 0 and is
 *     never selected.  Known limit, inherited from COUNT DISTINCT: the
 *     chain is a linked list, so the gather is serial in the chain length;
 *     cost is linear in the distinct values ever seen per key, because the
 *     append-only pool never reclaims zero-net nodes.
 *   - Changed-key tracking is a plain per-slot epoch store in the update
 *     kernel (idempotent, no atomics, same cache line as the state);
 *     flush scans the table for the current epoch -- a streaming read at
 *     HBM rate, paid at the control-rate flush cadence instead of adding
 *     list-append atomics to the per-row path.
 *   - Flush (the reference's handle_tick -> flush :637-737) evaluates each
 *     changed key, compares with the key's last-emitted values, and emits
 *     retract(last) + append(new) (retract-only on deletion, nothing when
 *     unchanged) through a wave-aggregated output cursor; the retract row
 *     always directly precedes its append row.
 *   - SQL NULLs are opt-in (AmdUpdatingConfig.null_semantics = 1): value
 *     columns arrive with Arrow validity bitmaps, k_updagg_update_nullable
 *     skips an aggregate's atomics where its argument is NULL and keeps a
 *     per-aggregate non-null count, flush decides NULL from that count (or
 *     from the condition under which the result is undefined) and emits a
 *     validity mask per row, and k_updagg_pack_validity ballots the masks
 *     into per-column Arrow bitmaps on the device.  With the option off
 *     the non-nullable kernels run, instantiated from the same source.
 *     The C oracle has no NULLs: tests/test_null_aggs.py compares against
 *     a Python model of DataFusion's accumulator rule.
 *   - Float64 value columns are opt-in per column
 *     (AmdUpdatingConfig.val_is_f64): the column's i64 plane holds f64 bit
 *     patterns.  An operator with a flagged column runs the *_f64 kernels,
 *     instantiated from the same source: SUM / AVG and the moment words
 *     fold with the hardware f64 atomic add, MIN / MAX and the order
 *     statistics use op_common.h's totalOrder encoding (so the radix
 *     select is unchanged), and a flush that finds a key empty zeroes its
 *     f64 sum words.  The rules are restated from DataFusion 48 /
 *     arrow-arith, not golden-pinned: the checker is the Python model
 *     tests/updagg_f64_ref.py (tests/test_updagg_f64.py).  Drain / restore
 *     carry state words raw; restoring into an operator with other flags
 *     is the caller's error.
 *
 * Parity is pinned against oracle/arroyo_oracle.c (itself pinned against
 * the reference's debezium_agg / filter_updating_aggregates golden
 * vectors) by tests/test_updagg.py.
 */
#include "op_common.h"

namespace updagg {

#define UERR_TABLE_FULL 1
#define UERR_POOL_FULL  2
#define UERR_OUT_CAP    3
#define UERR_RETRACT    4
#define UERR_ORD_ROWS   5   /* multiset total != live row count */
#define UERR_ORD_CHAIN  6   /* chain walk / scratch arena bound hit */

__host__ __device__ inline uint64_t enc_min(int64_t v) {
    return ~(((uint64_t)v) ^ 0x8000000000000000ULL);
}
__host__ __device__ inline int64_t dec_min(uint64_t e) {
    return (int64_t)((~e) ^ 0x8000000000000000ULL);
}
__host__ __device__ inline uint64_t enc_max(int64_t v) {
    return ((uint64_t)v) ^ 0x8000000000000000ULL;
}
__host__ __device__ inline int64_t dec_max(uint64_t e) {
    return (int64_t)(e ^ 0x8000000000000000ULL);
}

#define UAGG_MAX_SW 128  /* total state words cap per key */

struct AggSpec {
    int32_t n_aggs;
    int32_t op[AMD_MAX_AGGS];
    int32_t col[AMD_MAX_AGGS];
    int32_t col2[AMD_MAX_AGGS];  /* co-moment family second argument */
    int32_t soff[AMD_MAX_AGGS];  /* agg a's state words at st[soff[a]..] */
    int32_t SW;                  /* total state words per key */
    uint32_t f64m;               /* bit c: value column c holds f64 bit
                                    patterns; read by the F64 kernels only */
};

/* aggregate a's argument (col) / second argument (col2) column is f64 */
__host__ __device__ inline bool ua_f64_col(const AggSpec &agg, int col) {
    return col >= 0 && ((agg.f64m >> col) & 1);
}

/* distinct-value multiset node (append-only pool) */
struct Node {
    int64_t value;
    long long delta;      /* net refcount contribution (atomicAdd +-1) */
    int32_t next;
    int32_t pad;
};

struct UStore {
    int64_t *keys;        /* [C+1]; slot C = spec (key == EMPTY_KEY) */
    uint32_t *epoch;      /* [C+1] last-touched flush epoch */
    long long *rows;      /* [C+1] live row count (presence) */
    uint64_t *st;         /* [(C+1) * SW] scalar states (variable width) */
    int64_t *last;        /* [(C+1) * n_aggs] last emitted values */
    uint32_t *emitted;    /* [C+1] */
    int32_t *head;        /* [(C+1) * 8] value-multiset chains
                             (COUNT_DISTINCT, MEDIAN, MIN/MAX_RETRACT) */
    int64_t *ord;         /* [(C+1) * n_aggs] order-statistic results of the
                             current flush; null without an ordered agg */
    Node *pool;
    unsigned long long *pool_cur;
    int64_t pool_cap;
    uint32_t C;
};

__device__ inline int64_t ukey_slot(const UStore &S, int64_t key, int *err) {
    if (key == EMPTY_KEY) return (int64_t)S.C;
    uint64_t m = S.C - 1;
    uint64_t j = hash64((uint64_t)key) & m;
    for (uint32_t probes = 0; probes < S.C; probes++) {
        int64_t cur = S.keys[j];
        if (cur == key) return (int64_t)j;
        if (cur == EMPTY_KEY) {
            int64_t old = (int64_t)atomicCAS(
                (unsigned long long *)&S.keys[j],
                (unsigned long long)EMPTY_KEY, (unsigned long long)key);
            if (old == EMPTY_KEY || old == key) return (int64_t)j;
        }
        j = (j + 1) & m;
    }
    *err = UERR_TABLE_FULL;
    return -1;
}

/* add +-1 to value v's net refcount in the (slot, agg) chain.  Fields of a
 * new node are written before the atomicCAS publish (release via
 * __threadfence); walkers read them with volatile loads so a stale L1 line
 * covering a freshly-allocated neighbour node is never used. */
__device__ inline void chain_add(const UStore &S, int64_t slot, int agg,
                                 int64_t v, long long d, int *err) {
    int32_t *headp = &S.head[(size_t)slot * 8 + agg];
    for (int32_t j = *(volatile int32_t *)headp; j >= 0;) {
        volatile Node *n = (volatile Node *)&S.pool[j];
        if (n->value == v) {
            atomicAdd((unsigned long long *)&S.pool[j].delta,
                      (unsigned long long)d);
            return;
        }
        j = n->next;
    }
    int64_t idx = (int64_t)atomicAdd(S.pool_cur, 1ULL);
    if (idx >= S.pool_cap) { *err = UERR_POOL_FULL; return; }
    S.pool[idx].value = v;
    S.pool[idx].delta = d;
    /* the link is written BEFORE the node becomes reachable (CAS push): a
     * node published with its `next` still unset would send a concurrent
     * walker through whatever index the fresh pool memory holds, into some
     * other (key, aggregate)'s chain, where it could find v and add its
     * count to the wrong multiset */
    int32_t old = *(volatile int32_t *)headp;
    for (;;) {
        S.pool[idx].next = old;
        __threadfence();
        int32_t prev = atomicCAS(headp, old, (int32_t)idx);
        if (prev == old) break;
        old = prev;
    }
}

struct UpdateArgs {
    const int64_t *cols[12];   /* [key?], vals..., is_retract */
    int32_t n_keys, n_vals;
    int64_t n_rows;
    UStore store;
    AggSpec agg;
    uint32_t cur_epoch;
    int *err;
};

/* CAS-fold a double add (no f64 atomicAdd ordering requirements here;
 * contention is per (key, agg)) */
__device__ inline void fold_f64(uint64_t *w, double dv) {
    unsigned long long old = *w, assumed;
    do {
        assumed = old;
        double cur;
        memcpy(&cur, &assumed, 8);
        cur += dv;
        unsigned long long nv;
        memcpy(&nv, &cur, 8);
        old = atomicCAS((unsigned long long *)w, assumed, nv);
    } while (old != assumed);
}

/* The f64 add of the F64 kernels: the hardware global_atomic_add_f64 (no
 * return value, no retry loop).  The state plane is hipMalloc'ed
 * (coarse-grained) device memory, where the instruction is defined; under
 * key skew the 64 lanes of a wave that hit one word queue at the memory
 * side once instead of CAS-looping against each other
 * (profiles/updagg_f64_note.md). */
__device__ inline void add_f64(uint64_t *w, double dv) {
    unsafeAtomicAdd((double *)w, dv);
}

/* an aggregate's argument as a double: the bits themselves when its column
 * is flagged f64, the converted integer otherwise */
__device__ inline double ua_arg(bool isf, int64_t v) {
    double x;
    memcpy(&x, &v, 8);
    return isf ? x : (double)v;
}

/* ---- SQL NULL semantics (AmdUpdatingConfig.null_semantics == 1) ----
 *
 * Every aggregate keeps n_a, its count of live contributing rows (argument
 * non-null; both arguments for the co-moment family), in one state word:
 * COUNT(col) and AVG already hold it in st[0] (COUNT(*) counts every row,
 * so it reads the key's row count and keeps no state); the one-word and
 * chained states use their spare st[1]; the moment, co-moment and bit
 * states grow by one trailing word.  ua_noff is that word's offset within the aggregate's
 * state, ua_width the state width. */
__host__ __device__ inline bool ua_is_comoment(int op) {
    return op >= AMD_AGG_COVAR_POP && op <= AMD_AGG_REGR_SXY;
}
__host__ __device__ inline int ua_noff(int op) {
    if (op == AMD_AGG_COUNT || op == AMD_AGG_AVG) return 0;
    if (op >= AMD_AGG_STDDEV && op <= AMD_AGG_VAR_POP) return 2;
    if (ua_is_comoment(op)) return 5;
    if (op == AMD_AGG_BIT_AND || op == AMD_AGG_BIT_OR) return 32;
    return 1;
}
__host__ __device__ inline int ua_width(int op, int null_semantics) {
    int w = 2;
    if (ua_is_comoment(op)) w = 5;
    else if (op == AMD_AGG_BIT_AND || op == AMD_AGG_BIT_OR) w = 32;
    if (null_semantics && ua_noff(op) >= w) w = ua_noff(op) + 1;
    return w;
}

/* The update loop.  NS = false is the non-nullable kernel; NS = true reads
 * each value column's Arrow validity bitmap as 64-bit words (the 64
 * consecutive rows of a wavefront share one word per column: blocks are 256
 * threads and the grid stride a multiple of 256, so a wave's first row is a
 * multiple of 64), skips the atomics of an aggregate whose argument is
 * null, and counts the contributing rows in the aggregate's n_a word.
 * F64 = true is the kernel of an operator with at least one f64 value
 * column (AggSpec.f64m): SUM over such a column folds d * v as a double,
 * MIN / MAX use the float encodings, the moment families convert each
 * argument by its own column's flag, and every f64 fold is add_f64.  The
 * chained aggregates pass raw bits either way.  F64 = false is the i64
 * operator's code, untouched by the flags. */
template <bool NS, bool F64>
__device__ __forceinline__ void update_rows(const UpdateArgs &A,
                                            const uint64_t *const *valid) {
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t *retr = A.cols[A.n_keys + A.n_vals];
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         r < A.n_rows; r += stride) {
        int64_t key = A.n_keys ? A.cols[0][r] : 0;
        int64_t slot = ukey_slot(A.store, key, A.err);
        if (slot < 0) continue;
        long long d = retr[r] ? -1 : 1;
        A.store.epoch[slot] = A.cur_epoch;
        atomicAdd((unsigned long long *)&A.store.rows[slot],
                  (unsigned long long)d);
        unsigned vm = 0xFFu;   /* bit c: value column c is non-null */
        if constexpr (NS) {
            for (int c = 0; c < A.n_vals; c++) {
                const uint64_t *bm = valid[c];
                if (bm && !((bm[r >> 6] >> (r & 63)) & 1)) vm &= ~(1u << c);
            }
        }
        uint64_t *stp = A.store.st + (size_t)slot * A.agg.SW;
        for (int a = 0; a < A.agg.n_aggs; a++) {
            int64_t v = A.agg.col[a] >= 0
                            ? A.cols[A.n_keys + A.agg.col[a]][r] : 0;
            uint64_t *st = stp + A.agg.soff[a];
            if constexpr (NS) {
                int op = A.agg.op[a];
                /* COUNT(*) is the key's live row count, already kept in
                 * rows[slot]: no second atomic for it */
                if (op == AMD_AGG_COUNT && A.agg.col[a] < 0) continue;
                bool ok = A.agg.col[a] < 0 || ((vm >> A.agg.col[a]) & 1);
                if (ua_is_comoment(op))
                    ok = ok && ((vm >> A.agg.col2[a]) & 1);
                if (!ok) {
                    /* append-only MIN/MAX reject a retraction whatever the
                     * retracted value is */
                    if ((op == AMD_AGG_MIN || op == AMD_AGG_MAX) && d < 0)
                        *A.err = UERR_RETRACT;
                    continue;
                }
                /* COUNT and AVG count n_a in st[0] themselves */
                if (ua_noff(op) != 0)
                    atomicAdd((unsigned long long *)&st[ua_noff(op)],
                              (unsigned long long)d);
            }
            if constexpr (F64) {
                bool vf = ua_f64_col(A.agg, A.agg.col[a]);
                bool done = true;
                switch (A.agg.op[a]) {
                case AMD_AGG_SUM:
                    if (vf) add_f64(&st[0], (double)d * ua_arg(true, v));
                    else done = false;
                    break;
                case AMD_AGG_AVG:
                    atomicAdd((unsigned long long *)&st[0],
                              (unsigned long long)d);
                    add_f64(&st[1], (double)d * ua_arg(vf, v));
                    break;
                case AMD_AGG_MIN:
                    if (d < 0) { *A.err = UERR_RETRACT; break; }
                    atomicMax((unsigned long long *)&st[0],
                              (unsigned long long)(vf ? enc_minf(v)
                                                      : enc_min(v)));
                    break;
                case AMD_AGG_MAX:
                    if (d < 0) { *A.err = UERR_RETRACT; break; }
                    atomicMax((unsigned long long *)&st[0],
                              (unsigned long long)(vf ? enc_maxf(v)
                                                      : enc_max(v)));
                    break;
                case AMD_AGG_STDDEV:
                case AMD_AGG_STDDEV_POP:
                case AMD_AGG_VAR:
                case AMD_AGG_VAR_POP: {
                    double x = ua_arg(vf, v);
                    add_f64(&st[0], (double)d * x);
                    add_f64(&st[1], (double)d * x * x);
                    break;
                }
                case AMD_AGG_COVAR_POP: case AMD_AGG_COVAR_SAMP:
                case AMD_AGG_CORR: case AMD_AGG_REGR_SLOPE:
                case AMD_AGG_REGR_INTERCEPT: case AMD_AGG_REGR_R2:
                case AMD_AGG_REGR_AVGX: case AMD_AGG_REGR_AVGY:
                case AMD_AGG_REGR_COUNT: case AMD_AGG_REGR_SXX:
                case AMD_AGG_REGR_SYY: case AMD_AGG_REGR_SXY: {
                    double y = ua_arg(vf, v);
                    double x = ua_arg(
                        ua_f64_col(A.agg, A.agg.col2[a]),
                        A.cols[A.n_keys + A.agg.col2[a]][r]);
                    add_f64(&st[0], d * y);
                    add_f64(&st[1], d * x);
                    add_f64(&st[2], d * x * y);
                    add_f64(&st[3], d * y * y);
                    add_f64(&st[4], d * x * x);
                    break;
                }
                default:
                    done = false;
                    break;
                }
                if (done) continue;
            }
            switch (A.agg.op[a]) {
            case AMD_AGG_COUNT:
                atomicAdd((unsigned long long *)&st[0],
                          (unsigned long long)d);
                break;
            case AMD_AGG_SUM:
                atomicAdd((unsigned long long *)&st[0],
                          (unsigned long long)(d * v));
                break;
            case AMD_AGG_AVG:
                atomicAdd((unsigned long long *)&st[0],
                          (unsigned long long)d);
                fold_f64(&st[1], (double)d * (double)v);
                break;
            case AMD_AGG_MIN:
                if (d < 0) { *A.err = UERR_RETRACT; break; }
                atomicMax((unsigned long long *)&st[0],
                          (unsigned long long)enc_min(v));
                break;
            case AMD_AGG_MAX:
                if (d < 0) { *A.err = UERR_RETRACT; break; }
                atomicMax((unsigned long long *)&st[0],
                          (unsigned long long)enc_max(v));
                break;
            case AMD_AGG_COUNT_DISTINCT:
            case AMD_AGG_MEDIAN:
            case AMD_AGG_MIN_RETRACT:
            case AMD_AGG_MAX_RETRACT:
                chain_add(A.store, slot, a, v, d, A.err);
                break;
            case AMD_AGG_STDDEV:
            case AMD_AGG_STDDEV_POP:
            case AMD_AGG_VAR:
            case AMD_AGG_VAR_POP:
                fold_f64(&st[0], (double)d * (double)v);
                fold_f64(&st[1], (double)d * (double)v * (double)v);
                break;
            case AMD_AGG_BIT_XOR:
                atomicXor((unsigned long long *)&st[0],
                          (unsigned long long)v);
                break;
            case AMD_AGG_COVAR_POP: case AMD_AGG_COVAR_SAMP:
            case AMD_AGG_CORR: case AMD_AGG_REGR_SLOPE:
            case AMD_AGG_REGR_INTERCEPT: case AMD_AGG_REGR_R2:
            case AMD_AGG_REGR_AVGX: case AMD_AGG_REGR_AVGY:
            case AMD_AGG_REGR_COUNT: case AMD_AGG_REGR_SXX:
            case AMD_AGG_REGR_SYY: case AMD_AGG_REGR_SXY: {
                double y = (double)v;
                double x = (double)A.cols[A.n_keys + A.agg.col2[a]][r];
                fold_f64(&st[0], d * y);
                fold_f64(&st[1], d * x);
                fold_f64(&st[2], d * x * y);
                fold_f64(&st[3], d * y * y);
                fold_f64(&st[4], d * x * x);
                break;
            }
            case AMD_AGG_BIT_AND:
            case AMD_AGG_BIT_OR: {
                unsigned int *cnt = (unsigned int *)st;
                uint64_t uv = (uint64_t)v;
                unsigned int du = (unsigned int)(int)d;
                while (uv) {
                    int b = (int)(__ffsll((long long)uv) - 1);
                    atomicAdd(&cnt[b], du);  /* u32 wraps; net exact */
                    uv &= uv - 1;
                }
                break;
            }
            }
        }
    }
}

__global__ void __launch_bounds__(256)
k_updagg_update(UpdateArgs A) {
    update_rows<false, false>(A, nullptr);
}

__global__ void __launch_bounds__(256)
k_updagg_update_f64(UpdateArgs A) {
    update_rows<false, true>(A, nullptr);
}

struct UpdateArgsN {
    UpdateArgs A;
    const uint64_t *valid[8];  /* per value column; null = all valid */
};

__global__ void __launch_bounds__(256)
k_updagg_update_nullable(UpdateArgsN N) {
    update_rows<true, false>(N.A, N.valid);
}

__global__ void __launch_bounds__(256)
k_updagg_update_nullable_f64(UpdateArgsN N) {
    update_rows<true, true>(N.A, N.valid);
}

/* evaluate one key's current values into out[n_aggs] (i64 / f64-bits).
 * COUNT DISTINCT walks the chain, summing per-value deltas with an in-chain
 * dedup (duplicate nodes from racing first-inserts are rare and benign). */
/* NS (null semantics): n_a replaces the key's row count wherever an
 * aggregate uses n, *vmask gets bit a set when aggregate a is non-NULL, and
 * the value under a NULL is 0.  NULL is decided from the condition (n_a == 0
 * or the result undefined), never by testing the result for NaN.
 * F64: MIN / MAX over a flagged column decode with the float decoders; the
 * f64 SUM word is emitted as it stands, which is the i64 SUM's code. */
template <bool NS, bool F64>
__device__ inline void ueval_slot(const UStore &S, const AggSpec &agg,
                                  int64_t slot, int64_t *out,
                                  unsigned *vmask) {
    const uint64_t *stp = S.st + (size_t)slot * agg.SW;
    unsigned vm = 0;
    for (int a = 0; a < agg.n_aggs; a++) {
        const uint64_t *st = stp + agg.soff[a];
        bool ok = true;   /* NS: aggregate a is non-NULL */
        long long na_rows = 0;
        if constexpr (NS) na_rows = (long long)st[ua_noff(agg.op[a])];
        switch (agg.op[a]) {
        case AMD_AGG_COUNT:
            /* NS: COUNT(*) keeps no state of its own (see update_rows) */
            out[a] = NS && agg.col[a] < 0 ? (int64_t)S.rows[slot]
                                          : (int64_t)st[0];
            break;
        case AMD_AGG_SUM:
            out[a] = (int64_t)st[0];
            if constexpr (NS) ok = na_rows > 0;
            break;
        case AMD_AGG_MIN:
            out[a] = dec_min(st[0]);
            if constexpr (F64)
                if (ua_f64_col(agg, agg.col[a])) out[a] = dec_minf(st[0]);
            if constexpr (NS) ok = na_rows > 0;
            break;
        case AMD_AGG_MAX:
            out[a] = dec_max(st[0]);
            if constexpr (F64)
                if (ua_f64_col(agg, agg.col[a])) out[a] = dec_maxf(st[0]);
            if constexpr (NS) ok = na_rows > 0;
            break;
        case AMD_AGG_AVG: {
            double sum;
            uint64_t w1 = st[1];
            memcpy(&sum, &w1, 8);
            double v = sum / (double)(int64_t)st[0];
            memcpy(&out[a], &v, 8);
            if constexpr (NS) ok = na_rows > 0;
            break;
        }
        case AMD_AGG_STDDEV:
        case AMD_AGG_STDDEV_POP:
        case AMD_AGG_VAR:
        case AMD_AGG_VAR_POP: {
            double n = NS ? (double)na_rows : (double)S.rows[slot];
            double sx, sxx;
            uint64_t w0 = st[0], w1 = st[1];
            memcpy(&sx, &w0, 8);
            memcpy(&sxx, &w1, 8);
            double mean = sx / n;
            double m2 = sxx - n * mean * mean;
            if (m2 < 0.0) m2 = 0.0;
            int samp = agg.op[a] == AMD_AGG_STDDEV ||
                       agg.op[a] == AMD_AGG_VAR;
            double var = samp ? (n > 1.0 ? m2 / (n - 1.0) : NAN) : m2 / n;
            if (agg.op[a] == AMD_AGG_STDDEV ||
                agg.op[a] == AMD_AGG_STDDEV_POP)
                var = sqrt(var);
            memcpy(&out[a], &var, 8);
            if constexpr (NS) ok = samp ? n > 1.0 : n > 0.0;
            break;
        }
        case AMD_AGG_BIT_XOR:
            out[a] = (int64_t)st[0];
            if constexpr (NS) ok = na_rows > 0;
            break;
        case AMD_AGG_COVAR_POP: case AMD_AGG_COVAR_SAMP:
        case AMD_AGG_CORR: case AMD_AGG_REGR_SLOPE:
        case AMD_AGG_REGR_INTERCEPT: case AMD_AGG_REGR_R2:
        case AMD_AGG_REGR_AVGX: case AMD_AGG_REGR_AVGY:
        case AMD_AGG_REGR_COUNT: case AMD_AGG_REGR_SXX:
        case AMD_AGG_REGR_SYY: case AMD_AGG_REGR_SXY: {
            double n = NS ? (double)na_rows : (double)S.rows[slot];
            double w[5];
            for (int k = 0; k < 5; k++) {
                uint64_t b = st[k];
                memcpy(&w[k], &b, 8);
            }
            double my = w[0] / n, mx = w[1] / n;
            double Sxy = w[2] - n * mx * my;
            double Syy = w[3] - n * my * my;
            double Sxx = w[4] - n * mx * mx;
            if (Sxx < 0.0) Sxx = 0.0;
            if (Syy < 0.0) Syy = 0.0;
            double v;
            switch (agg.op[a]) {
            case AMD_AGG_COVAR_POP:  v = Sxy / n; break;
            case AMD_AGG_COVAR_SAMP:
                v = n > 1.0 ? Sxy / (n - 1.0) : NAN;
                break;
            case AMD_AGG_CORR:
                v = (n > 1.0 && Sxx > 0.0 && Syy > 0.0)
                        ? Sxy / sqrt(Sxx * Syy) : NAN;
                break;
            case AMD_AGG_REGR_SLOPE:
                v = Sxx > 0.0 ? Sxy / Sxx : NAN;
                break;
            case AMD_AGG_REGR_INTERCEPT:
                v = Sxx > 0.0 ? my - (Sxy / Sxx) * mx : NAN;
                break;
            case AMD_AGG_REGR_R2:
                v = Sxx <= 0.0 ? NAN
                    : (Syy <= 0.0 ? 1.0 : (Sxy * Sxy) / (Sxx * Syy));
                break;
            case AMD_AGG_REGR_AVGX: v = mx; break;
            case AMD_AGG_REGR_AVGY: v = my; break;
            case AMD_AGG_REGR_SXX: v = Sxx; break;
            case AMD_AGG_REGR_SYY: v = Syy; break;
            case AMD_AGG_REGR_SXY: v = Sxy; break;
            default: v = 0.0; break;
            }
            if (agg.op[a] == AMD_AGG_REGR_COUNT)
                out[a] = NS ? (int64_t)na_rows : (int64_t)S.rows[slot];
            else
                memcpy(&out[a], &v, 8);
            if constexpr (NS) {
                /* the conditions under which v above is the NaN filler */
                switch (agg.op[a]) {
                case AMD_AGG_REGR_COUNT: break;
                case AMD_AGG_COVAR_SAMP: ok = n > 1.0; break;
                case AMD_AGG_CORR:
                    ok = n > 1.0 && Sxx > 0.0 && Syy > 0.0;
                    break;
                case AMD_AGG_REGR_SLOPE:
                case AMD_AGG_REGR_INTERCEPT:
                case AMD_AGG_REGR_R2:
                    ok = n > 0.0 && Sxx > 0.0;
                    break;
                default: ok = n > 0.0; break;
                }
            }
            break;
        }
        case AMD_AGG_BIT_AND:
        case AMD_AGG_BIT_OR: {
            const unsigned int *cnt = (const unsigned int *)st;
            long long rows = NS ? na_rows : S.rows[slot];
            uint64_t r2 = 0;
            for (int b = 0; b < 64; b++) {
                unsigned int nb = cnt[b];
                int set = agg.op[a] == AMD_AGG_BIT_AND
                              ? (long long)nb == rows && rows > 0
                              : nb > 0;
                if (set) r2 |= 1ULL << b;
            }
            out[a] = (int64_t)r2;
            if constexpr (NS) ok = rows > 0;
            break;
        }
        case AMD_AGG_COUNT_DISTINCT: {
            int64_t cnt = 0;
            int32_t headv = *(volatile int32_t *)
                &S.head[(size_t)slot * 8 + a];
            for (int32_t i = headv; i >= 0;) {
                volatile Node *ni = (volatile Node *)&S.pool[i];
                int64_t v = ni->value;
                /* first occurrence of v in the chain? */
                bool first = true;
                long long total = ni->delta;
                for (int32_t j = headv; j != i;) {
                    volatile Node *nj = (volatile Node *)&S.pool[j];
                    if (nj->value == v) { first = false; break; }
                    j = nj->next;
                }
                if (first) {
                    for (int32_t j = ni->next; j >= 0;) {
                        volatile Node *nj = (volatile Node *)&S.pool[j];
                        if (nj->value == v) total += nj->delta;
                        j = nj->next;
                    }
                    if (total > 0) cnt++;
                }
                i = ni->next;
            }
            out[a] = cnt;
            break;
        }
        case AMD_AGG_MEDIAN:
        case AMD_AGG_MIN_RETRACT:
        case AMD_AGG_MAX_RETRACT:
            /* selected by k_updagg_ordstat earlier in this flush, for
             * exactly the slots that reach this point (NS: for the
             * (slot, aggregate) pairs with n_a > 0) */
            if constexpr (NS) ok = na_rows > 0;
            if (ok) out[a] = S.ord[(size_t)slot * agg.n_aggs + a];
            break;
        }
        if constexpr (NS) {
            if (ok) vm |= 1u << a;
            else out[a] = 0;
        }
    }
    if constexpr (NS) *vmask = vm;
}

/* ---- order statistics (MEDIAN, MIN_RETRACT, MAX_RETRACT) at flush ----
 *
 * One wavefront per changed (slot, ordered aggregate).  LDS per wave: a
 * tile of UORD_TILE (encoded value, net count) entries = 256 * 16 B = 4 KB,
 * plus a 256-bin i64 histogram = 2 KB; a 256-thread workgroup (4 waves)
 * holds 24 KB, so LDS admits 6 workgroups = 24 waves per CU of the 160 KB.
 * Chains with more than UORD_TILE live nodes go to a global arena of
 * pool_cap entries: every chain is visited once per flush and chains are
 * disjoint, so a per-flush bump allocation cannot exceed the pool size. */
#define UORD_TILE 256
#define UORD_WAVES 4

struct OrdEnt {
    uint64_t enc;         /* enc_max(value): unsigned order == i64 order */
    long long net;        /* this node's share of the value's refcount */
};

struct OrdArgs {
    UStore store;
    AggSpec agg;
    uint32_t cur_epoch;
    OrdEnt *arena;
    unsigned long long *arena_cur;
    int64_t arena_cap;
    int *err;
};

/* one wave's LDS phases are ordered by this; waves of a workgroup run
 * independent trip counts, so no workgroup barrier may be used here */
__device__ __forceinline__ void wave_sync() {
    __threadfence_block();
    __builtin_amdgcn_wave_barrier();
}

/* Element of rank r (0-based) of the multiset {ent[i].enc weighted by
 * ent[i].net}, by MSB-first radix select.  Every loop is bounded by n or a
 * constant whatever the weights are; *bad is set when no bin holds r
 * (possible only when a value's summed net is negative).  All entries agree
 * on the bytes above ptop (prefix0 holds them), so the passes start at byte
 * ptop; ptop < 0 means a single value. */
__device__ __forceinline__ uint64_t ord_select(const volatile OrdEnt *ent,
                                               int64_t n, long long r,
                                               uint64_t prefix0, int ptop,
                                               long long *hist, int lane,
                                               bool *bad) {
    uint64_t prefix = prefix0;
    for (int p = ptop; p >= 0; p--) {
        int sh = p * 8;
        uint64_t himask = p == 7 ? 0ULL : ~0ULL << (sh + 8);
        for (int b = lane; b < 256; b += 64) hist[b] = 0;
        wave_sync();
        for (int64_t i = lane; i < n; i += 64) {
            uint64_t e = ent[i].enc;
            long long w = ent[i].net;
            if (((e ^ prefix) & himask) == 0)
                atomicAdd((unsigned long long *)&hist[(e >> sh) & 255],
                          (unsigned long long)w);
        }
        wave_sync();
        /* lane l owns bins 4l..4l+3; wave-wide inclusive scan of the sums */
        long long b[4], s = 0;
        for (int k = 0; k < 4; k++) {
            b[k] = hist[lane * 4 + k];
            s += b[k];
        }
        long long inc = s;
        for (int o = 1; o < 64; o <<= 1) {
            long long t = __shfl_up(inc, o, 64);
            if (lane >= o) inc += t;
        }
        long long c = inc - s;
        int dsel = -1;
        long long rsel = 0;
        for (int k = 0; k < 4; k++) {
            if (dsel < 0 && r >= c && r < c + b[k]) {
                dsel = lane * 4 + k;
                rsel = r - c;
            }
            c += b[k];
        }
        unsigned long long m = __ballot(dsel >= 0);
        wave_sync();   /* hist is rewritten by the next pass */
        if (!m) {
            *bad = true;
            return prefix;
        }
        int src = (int)__ffsll((long long)m) - 1;
        int d = __shfl(dsel, src, 64);
        r = __shfl(rsel, src, 64);
        prefix |= (uint64_t)d << sh;
    }
    return prefix;
}

/* encoded word <-> raw value of a chained aggregate: enc_max order for an
 * i64 column, the totalOrder float encoding for an f64 one */
__device__ __forceinline__ uint64_t ord_enc(bool isf, int64_t v) {
    return isf ? enc_maxf(v) : enc_max(v);
}
__device__ __forceinline__ int64_t ord_dec(bool isf, uint64_t e) {
    return isf ? dec_maxf(e) : dec_max(e);
}

/* even-count median of an f64 column: (lo + hi) / 2.0, an IEEE add then an
 * IEEE divide (DataFusion's); lo + hi may overflow to inf, NaN propagates */
__device__ inline int64_t ord_midpoint_f64(int64_t lo, int64_t hi) {
    double a, b;
    memcpy(&a, &lo, 8);
    memcpy(&b, &hi, 8);
    double m = (a + b) / 2.0;
    int64_t r;
    memcpy(&r, &m, 8);
    return r;
}

/* (lo + hi) / 2 truncated toward zero, without 64-bit overflow */
__host__ __device__ inline int64_t ord_midpoint(int64_t lo, int64_t hi) {
    int64_t s = lo / 2 + hi / 2;
    int rr = (int)(lo % 2) + (int)(hi % 2);   /* -2..2 */
    if (rr == 2) return s + 1;
    if (rr == -2) return s - 1;
    if (rr == 1) return s >= 0 ? s : s + 1;
    if (rr == -1) return s > 0 ? s - 1 : s;
    return s;
}

/* NS: a (slot, aggregate) pair is selected when n_a > 0 (a key can have live
 * rows that are all NULL in the column: no select, no error) and the
 * multiset total is checked against n_a instead of the key's row count.
 * F64: an aggregate over a flagged column gathers with the float encoding
 * (the select and the shared-prefix skip work on encoded words and do not
 * change); only the decode and the even-count midpoint differ. */
template <bool NS, bool F64>
__device__ __forceinline__ void ordstat_body(const OrdArgs &A,
                                             OrdEnt (*tile_all)[UORD_TILE],
                                             long long (*hist_all)[256]) {
    const UStore &S = A.store;
    int na = A.agg.n_aggs;
    int lane = (int)(threadIdx.x & 63);
    int wv = (int)(threadIdx.x >> 6);
    OrdEnt *tile = tile_all[wv];
    long long *hist = hist_all[wv];
    /* per-op bit masks over the aggregate index (no indexed reads of the
     * kernel-argument arrays by a lane-varying index) */
    unsigned med = 0, mn = 0, mx = 0, fm = 0;
    for (int k = 0; k < AMD_MAX_AGGS; k++) {
        if (k >= na) break;
        if constexpr (F64)
            if (ua_f64_col(A.agg, A.agg.col[k])) fm |= 1u << k;
        if (A.agg.op[k] == AMD_AGG_MEDIAN) med |= 1u << k;
        if (A.agg.op[k] == AMD_AGG_MIN_RETRACT) mn |= 1u << k;
        if (A.agg.op[k] == AMD_AGG_MAX_RETRACT) mx |= 1u << k;
    }
    unsigned ordm = med | mn | mx;
    int64_t n_slots = (int64_t)S.C + 1;
    int64_t wave_id = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / 64;
    int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) / 64;
    /* a wave scans 8 slots x 8 aggregate columns per step: lane = (slot
     * offset, aggregate), the layout of the head plane.  Untouched slots
     * are rejected on the epoch word alone. */
    int sub = lane >> 3, la = lane & 7;
    /* this lane's n_a word: the chained states keep it at st[soff + 1] */
    int lnoff = 0;
    if constexpr (NS)
        for (int k = 0; k < AMD_MAX_AGGS; k++)
            if (k == la) lnoff = A.agg.soff[k] + 1;
    for (int64_t ws = wave_id * 8; ws < n_slots; ws += n_waves * 8) {
        int64_t lslot = ws + sub;
        bool want = false;
        int32_t lhead = -1;
        long long lrows = 0;   /* the live count the multiset must total */
        if (lslot < n_slots && ((ordm >> la) & 1) &&
            S.epoch[lslot] == A.cur_epoch &&
            (lslot == (int64_t)S.C || S.keys[lslot] != EMPTY_KEY)) {
            lrows = NS ? (long long)S.st[(size_t)lslot * A.agg.SW + lnoff]
                       : S.rows[lslot];
            if (lrows > 0) {
                want = true;
                lhead = S.head[(size_t)lslot * 8 + la];
            }
        }
        unsigned long long todo = __ballot(want);
        while (todo) {
            int src = (int)__ffsll((long long)todo) - 1;
            todo &= todo - 1;
            int64_t slot = ws + (src >> 3);
            int a = src & 7;
            bool isf = F64 && ((fm >> a) & 1);
            int32_t head = __shfl(lhead, src, 64);
            long long rows = __shfl(lrows, src, 64);
            /* gather: every lane walks the same chain (broadcast loads),
             * lane 0 stores the live nodes.  Steps are bounded by the
             * pool size and every index is range-checked, so a corrupt
             * link ends the walk instead of running away. */
            int64_t n = 0, steps = 0;
            long long W = 0;
            uint64_t first = 0, diff = 0;   /* bits in which entries differ */
            bool bad = false;
            for (int32_t j = head; j >= 0;) {
                if ((int64_t)j >= S.pool_cap || steps >= S.pool_cap) {
                    bad = true;
                    break;
                }
                steps++;
                int64_t v = S.pool[j].value;
                long long d = S.pool[j].delta;
                j = S.pool[j].next;
                if (d == 0) continue;          /* fully retracted value */
                uint64_t e = ord_enc(isf, v);
                if (n < UORD_TILE && lane == 0) {
                    tile[n].enc = e;
                    tile[n].net = d;
                }
                if (n == 0) first = e;
                diff |= e ^ first;
                W += d;
                n++;
            }
            const volatile OrdEnt *ent = tile;
            if (!bad && n > UORD_TILE) {
                /* wide chain: second walk into the global arena */
                unsigned long long base = 0;
                if (lane == 0)
                    base = atomicAdd(A.arena_cur, (unsigned long long)n);
                base = (unsigned long long)__shfl((long long)base, 0, 64);
                if ((int64_t)base + n > A.arena_cap) {
                    bad = true;
                } else {
                    OrdEnt *dst = A.arena + base;
                    int64_t i = 0;
                    steps = 0;
                    for (int32_t j = head; j >= 0 && i < n;) {
                        if ((int64_t)j >= S.pool_cap ||
                            steps >= S.pool_cap) {
                            bad = true;
                            break;
                        }
                        steps++;
                        int64_t v = S.pool[j].value;
                        long long d = S.pool[j].delta;
                        j = S.pool[j].next;
                        if (d == 0) continue;
                        if (lane == 0) {
                            dst[i].enc = ord_enc(isf, v);
                            dst[i].net = d;
                        }
                        i++;
                    }
                    if (i != n) bad = true;
                    __threadfence();
                    ent = dst;
                }
            }
            wave_sync();
            int64_t res = 0;
            if (bad) {
                if (lane == 0) *A.err = UERR_ORD_CHAIN;
            } else if (W != rows) {
                /* W <= 0 lands here too: rows > 0 for every slot taken */
                if (lane == 0) *A.err = UERR_ORD_ROWS;
            } else {
                bool sbad = false;
                /* skip the radix passes over bytes every entry shares
                 * (small-range columns differ in the low byte or two) */
                int ptop = diff ? (63 - __clzll((long long)diff)) >> 3 : -1;
                uint64_t pre =
                    ptop == 7 ? 0ULL : first & (~0ULL << ((ptop + 1) * 8));
                if ((mn >> a) & 1) {
                    res = ord_dec(isf, ord_select(ent, n, 0, pre, ptop, hist,
                                                  lane, &sbad));
                } else if ((mx >> a) & 1) {
                    res = ord_dec(isf, ord_select(ent, n, W - 1, pre, ptop,
                                                  hist, lane, &sbad));
                } else {
                    int64_t hi =
                        ord_dec(isf, ord_select(ent, n, W / 2, pre, ptop,
                                                hist, lane, &sbad));
                    res = hi;
                    if (!(W & 1)) {
                        int64_t lo =
                            ord_dec(isf, ord_select(ent, n, (W - 1) / 2, pre,
                                                    ptop, hist, lane, &sbad));
                        res = isf ? ord_midpoint_f64(lo, hi)
                                  : ord_midpoint(lo, hi);
                    }
                }
                if (sbad && lane == 0) *A.err = UERR_ORD_ROWS;
            }
            if (lane == 0) S.ord[(size_t)slot * na + a] = res;
            wave_sync();   /* tile is rewritten by the next item */
        }
    }
}

__global__ void __launch_bounds__(64 * UORD_WAVES)
k_updagg_ordstat(OrdArgs A) {
    __shared__ OrdEnt tile_all[UORD_WAVES][UORD_TILE];
    __shared__ long long hist_all[UORD_WAVES][256];
    ordstat_body<false, false>(A, tile_all, hist_all);
}

__global__ void __launch_bounds__(64 * UORD_WAVES)
k_updagg_ordstat_f64(OrdArgs A) {
    __shared__ OrdEnt tile_all[UORD_WAVES][UORD_TILE];
    __shared__ long long hist_all[UORD_WAVES][256];
    ordstat_body<false, true>(A, tile_all, hist_all);
}

__global__ void __launch_bounds__(64 * UORD_WAVES)
k_updagg_ordstat_nullable(OrdArgs A) {
    __shared__ OrdEnt tile_all[UORD_WAVES][UORD_TILE];
    __shared__ long long hist_all[UORD_WAVES][256];
    ordstat_body<true, false>(A, tile_all, hist_all);
}

__global__ void __launch_bounds__(64 * UORD_WAVES)
k_updagg_ordstat_nullable_f64(OrdArgs A) {
    __shared__ OrdEnt tile_all[UORD_WAVES][UORD_TILE];
    __shared__ long long hist_all[UORD_WAVES][256];
    ordstat_body<true, true>(A, tile_all, hist_all);
}

/* f64 subtraction is not exact: a key whose rows were all retracted (1e16,
 * 1.0, -1e16, -1.0 leaves -1.0) would hand the residue to its next life.
 * The reference drops the key's accumulators at the flush that finds it
 * empty (incremental_aggregator.rs:671-686); here that flush puts the sum
 * words fed by an f64 column back to +0.0.  The counts (n_a, AVG's count)
 * are integers and already 0.  k_updagg_expire clears the whole state. */
__device__ inline void ua_reset_f64(const UStore &S, const AggSpec &agg,
                                    int64_t slot) {
    uint64_t *stp = S.st + (size_t)slot * agg.SW;
    for (int a = 0; a < agg.n_aggs; a++) {
        uint64_t *st = stp + agg.soff[a];
        int op = agg.op[a];
        bool vf = ua_f64_col(agg, agg.col[a]);
        if (op == AMD_AGG_SUM && vf) {
            st[0] = 0;
        } else if (op == AMD_AGG_AVG && vf) {
            st[1] = 0;
        } else if (op >= AMD_AGG_STDDEV && op <= AMD_AGG_VAR_POP && vf) {
            st[0] = st[1] = 0;
        } else if (ua_is_comoment(op) &&
                   (vf || ua_f64_col(agg, agg.col2[a]))) {
            for (int k = 0; k < 5; k++) st[k] = 0;
        }
    }
}

struct FlushArgs {
    UStore store;
    AggSpec agg;
    uint32_t cur_epoch;
    int32_t n_keys;
    int64_t *out[AMD_MAX_AGGS + 2];
    unsigned long long *n_out;
    int64_t out_cap;
    int *err;
    /* null semantics only */
    uint32_t *lastv;      /* [C+1] validity mask of the last emitted row */
    uint32_t *vmask;      /* [out_cap] validity mask per emitted row */
};

/* NS: a flush decision compares (validity, value) per aggregate -- NULL
 * equals NULL and differs from every value (the value plane under a NULL is
 * 0, so mask equality plus value equality is exactly that) -- and every
 * emitted row carries its validity mask: bit a set = aggregate a non-NULL.
 * Retract rows re-emit the mask that was emitted with the row they retract.
 * F64: a touched key with zero live rows gets its f64-fed sum words reset
 * (ua_reset_f64); the unchanged-value test stays a bit compare. */
template <bool NS, bool F64>
__device__ __forceinline__ void flush_body(const FlushArgs &F) {
    const UStore &S = F.store;
    int na = F.agg.n_aggs;
    int lane = (int)(threadIdx.x & 63);
    /* whole wave iterates together (uniform trip count) so the output
     * cursor claim can be aggregated to one atomicAdd per wave */
    int64_t wave_id = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / 64;
    int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) / 64;
    for (int64_t ws = wave_id * 64; ws <= (int64_t)S.C;
         ws += n_waves * 64) {
        int64_t slot = ws + lane;
        int nr = 0;
        int64_t cur[AMD_MAX_AGGS];
        unsigned curv = 0;
        int64_t key = 0;
        bool do_retract = false, do_append = false;
        if (slot <= (int64_t)S.C && S.epoch[slot] == F.cur_epoch &&
            (slot == (int64_t)S.C ? true : S.keys[slot] != EMPTY_KEY)) {
            key = slot == (int64_t)S.C ? EMPTY_KEY : S.keys[slot];
            long long rows = S.rows[slot];
            if (rows > 0) ueval_slot<NS, F64>(S, F.agg, slot, cur, &curv);
            if constexpr (F64)
                if (rows == 0) ua_reset_f64(S, F.agg, slot);
            if (S.emitted[slot]) {
                bool same = rows > 0;
                if constexpr (NS) same = same && curv == F.lastv[slot];
                if (same)
                    for (int a = 0; a < na; a++)
                        if (cur[a] != S.last[(size_t)slot * na + a]) {
                            same = false;
                            break;
                        }
                if (!same) {
                    do_retract = true;
                    if (rows > 0) do_append = true;
                }
            } else if (rows > 0) {
                do_append = true;
            }
            nr = (do_retract ? 1 : 0) + (do_append ? 1 : 0);
        }
        /* wave-aggregated cursor claim: one atomicAdd per wave */
        unsigned long long act = __ballot(1);
        int total = 0;
        int prefix = 0;
        for (int l = 0; l < 64; l++) {
            int c = __shfl(nr, l, 64);
            if (!((act >> l) & 1)) c = 0;
            if (l < lane) prefix += c;
            total += c;
        }
        unsigned long long wbase = 0;
        int leader = (int)__ffsll((long long)act) - 1;
        if (lane == leader && total)
            wbase = atomicAdd(F.n_out, (unsigned long long)total);
        wbase = (unsigned long long)__shfl((long long)wbase, leader, 64);
        if (nr) {
            int64_t r = (int64_t)wbase + prefix;
            if (r + nr > F.out_cap) { *F.err = UERR_OUT_CAP; continue; }
            if (do_retract) {
                int col = 0;
                if (F.n_keys) F.out[col++][r] = key;
                for (int a = 0; a < na; a++)
                    F.out[col++][r] = S.last[(size_t)slot * na + a];
                F.out[col][r] = 1;
                if constexpr (NS) F.vmask[r] = F.lastv[slot];
                r++;
            }
            if (do_append) {
                int col = 0;
                if (F.n_keys) F.out[col++][r] = key;
                for (int a = 0; a < na; a++) {
                    F.out[col++][r] = cur[a];
                    S.last[(size_t)slot * na + a] = cur[a];
                }
                F.out[col][r] = 0;
                if constexpr (NS) {
                    F.vmask[r] = curv;
                    F.lastv[slot] = curv;
                }
                S.emitted[slot] = 1;
            } else if (do_retract) {
                S.emitted[slot] = 0;
            }
        }
    }
}

__global__ void __launch_bounds__(256)
k_updagg_flush(FlushArgs F) {
    flush_body<false, false>(F);
}

__global__ void __launch_bounds__(256)
k_updagg_flush_f64(FlushArgs F) {
    flush_body<false, true>(F);
}

__global__ void __launch_bounds__(256)
k_updagg_flush_nullable(FlushArgs F) {
    flush_body<true, false>(F);
}

__global__ void __launch_bounds__(256)
k_updagg_flush_nullable_f64(FlushArgs F) {
    flush_body<true, true>(F);
}

/* Per-row validity masks -> per-aggregate Arrow validity bitmaps.  One
 * wave's __ballot of "row valid in aggregate a" is the little-endian 64-bit
 * bitmap word of those 64 rows; lanes past n_rows vote 0, so the padding
 * bits of the last word are clear.  nullcols gets bit a when aggregate a has
 * at least one NULL row: only those bitmaps cross to the host. */
struct PackArgs {
    const uint32_t *vmask;
    int64_t n_rows;
    int32_t n_aggs;
    uint64_t *bm[AMD_MAX_AGGS];   /* [(n_rows + 63) / 64] words each */
    unsigned int *nullcols;
};

__global__ void __launch_bounds__(256)
k_updagg_pack_validity(PackArgs P) {
    int lane = (int)(threadIdx.x & 63);
    int64_t wave_id = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) / 64;
    int64_t n_waves = ((int64_t)gridDim.x * blockDim.x) / 64;
    /* wave-uniform trip count: every lane reaches every __ballot */
    for (int64_t base = wave_id * 64; base < P.n_rows; base += n_waves * 64) {
        int64_t r = base + lane;
        bool in = r < P.n_rows;
        unsigned vm = in ? P.vmask[r] : 0u;
        unsigned long long full = __ballot(in);
        for (int a = 0; a < P.n_aggs; a++) {
            unsigned long long w = __ballot(in && ((vm >> a) & 1));
            if (lane == 0) {
                P.bm[a][base >> 6] = w;
                /* the flag saturates: look before joining the queue on
                 * one address that every wave with a NULL would form */
                if (w != full &&
                    !((*(volatile unsigned int *)P.nullcols >> a) & 1))
                    atomicOr(P.nullcols, 1u << a);
            }
        }
    }
}

/* TTL eviction (the reference's UpdatingCache::time_out, epoch-based here;
 * see oracle).  Evicted keys emit retract(last) and reset in place: the
 * key slot stays claimed (open addressing), its distinct-value chain nodes
 * are orphaned in the append-only pool (bounded by log2_nodes; a loud
 * pool-full error, not silent corruption). */
struct ExpireArgs {
    UStore store;
    AggSpec agg;
    uint32_t cur_epoch;
    uint32_t idle;
    int32_t n_keys;
    int64_t *out[AMD_MAX_AGGS + 2];
    unsigned long long *n_out;
    int64_t out_cap;
    int *err;
    /* null semantics only (null pointers otherwise) */
    uint32_t *lastv;
    uint32_t *vmask;
};

__global__ void __launch_bounds__(256)
k_updagg_expire(ExpireArgs E) {
    const UStore &S = E.store;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    int na = E.agg.n_aggs;
    for (int64_t slot = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         slot <= (int64_t)S.C; slot += stride) {
        if (slot < (int64_t)S.C && S.keys[slot] == EMPTY_KEY) continue;
        uint32_t te = S.epoch[slot];
        if (te == 0 || E.cur_epoch - te <= E.idle) continue;
        if (!S.emitted[slot] && S.rows[slot] == 0) continue;
        if (S.emitted[slot]) {
            int64_t r = (int64_t)atomicAdd(E.n_out, 1ULL);
            if (r >= E.out_cap) { *E.err = UERR_OUT_CAP; continue; }
            int col = 0;
            if (E.n_keys)
                E.out[col++][r] =
                    slot == (int64_t)S.C ? EMPTY_KEY : S.keys[slot];
            for (int a = 0; a < na; a++)
                E.out[col++][r] = S.last[(size_t)slot * na + a];
            E.out[col][r] = 1;
            if (E.vmask) E.vmask[r] = E.lastv[slot];
        }
        S.emitted[slot] = 0;
        S.rows[slot] = 0;
        for (int w = 0; w < E.agg.SW; w++)
            S.st[(size_t)slot * E.agg.SW + w] = 0;
        for (int a = 0; a < na; a++) S.head[(size_t)slot * 8 + a] = -1;
    }
}

/* checkpoint drain which=0: scalar rows
 * [key?, rows, st words..., emitted, last...] plus, under null semantics, a
 * trailing last-emitted validity mask column (the per-aggregate n_a counts
 * are st words); which=1: multiset rows [key?, agg_index, value, net_count] */
struct UDrainArgs {
    UStore store;
    AggSpec agg;
    int32_t n_keys, which;
    int64_t *out[UAGG_MAX_SW + AMD_MAX_AGGS + 4];
    unsigned long long *n_out;
    int64_t out_cap;
    int *err;
    const uint32_t *lastv;   /* null semantics only (null otherwise) */
};

__global__ void __launch_bounds__(256)
k_updagg_drain(UDrainArgs D) {
    const UStore &S = D.store;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    int na = D.agg.n_aggs;
    for (int64_t slot = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         slot <= (int64_t)S.C; slot += stride) {
        if (slot < (int64_t)S.C && S.keys[slot] == EMPTY_KEY) continue;
        if (slot == (int64_t)S.C && S.rows[slot] == 0 && !S.emitted[slot])
            continue;
        int64_t key = slot == (int64_t)S.C ? EMPTY_KEY : S.keys[slot];
        if (D.which == 0) {
            int64_t r = (int64_t)atomicAdd(D.n_out, 1ULL);
            if (r >= D.out_cap) { *D.err = UERR_OUT_CAP; continue; }
            int col = 0;
            if (D.n_keys) D.out[col++][r] = key;
            D.out[col++][r] = (int64_t)S.rows[slot];
            for (int w = 0; w < D.agg.SW; w++)
                D.out[col++][r] =
                    (int64_t)S.st[(size_t)slot * D.agg.SW + w];
            D.out[col++][r] = (int64_t)S.emitted[slot];
            for (int a = 0; a < na; a++)
                D.out[col++][r] = S.last[(size_t)slot * na + a];
            if (D.lastv) D.out[col++][r] = (int64_t)D.lastv[slot];
        } else {
            for (int a = 0; a < na; a++) {
                if (D.agg.op[a] != AMD_AGG_COUNT_DISTINCT &&
                    D.agg.op[a] != AMD_AGG_MEDIAN &&
                    D.agg.op[a] != AMD_AGG_MIN_RETRACT &&
                    D.agg.op[a] != AMD_AGG_MAX_RETRACT)
                    continue;
                for (int32_t i = S.head[(size_t)slot * 8 + a]; i >= 0;
                     i = S.pool[i].next) {
                    if (S.pool[i].delta == 0) continue;
                    int64_t r = (int64_t)atomicAdd(D.n_out, 1ULL);
                    if (r >= D.out_cap) { *D.err = UERR_OUT_CAP; continue; }
                    int col = 0;
                    if (D.n_keys) D.out[col++][r] = key;
                    D.out[col++][r] = a;
                    D.out[col++][r] = S.pool[i].value;
                    D.out[col][r] = (int64_t)S.pool[i].delta;
                }
            }
        }
    }
}

/* restore which=0: one thread per row writes the slot's scalar state (each
 * key appears once in drained data); which=1: chain-insert value rows */
struct URestoreArgs {
    const int64_t *cols[UAGG_MAX_SW + AMD_MAX_AGGS + 4];
    int32_t n_cols;
    int64_t n_rows;
    UStore store;
    AggSpec agg;
    int32_t n_keys, which;
    int *err;
    uint32_t *lastv;         /* null semantics only (null otherwise) */
};

__global__ void __launch_bounds__(256)
k_updagg_restore(URestoreArgs R) {
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    int na = R.agg.n_aggs;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         r < R.n_rows; r += stride) {
        int64_t key = R.n_keys ? R.cols[0][r] : 0;
        int64_t slot = ukey_slot(R.store, key, R.err);
        if (slot < 0) continue;
        if (R.which == 0) {
            int col = R.n_keys;
            R.store.rows[slot] = (long long)R.cols[col++][r];
            for (int w = 0; w < R.agg.SW; w++)
                R.store.st[(size_t)slot * R.agg.SW + w] =
                    (uint64_t)R.cols[col++][r];
            R.store.emitted[slot] = (uint32_t)R.cols[col++][r];
            for (int a = 0; a < na; a++)
                R.store.last[(size_t)slot * na + a] = R.cols[col++][r];
            if (R.lastv) R.lastv[slot] = (uint32_t)R.cols[col++][r];
        } else {
            int a = (int)R.cols[R.n_keys][r];
            chain_add(R.store, slot, a, R.cols[R.n_keys + 1][r],
                      (long long)R.cols[R.n_keys + 2][r], R.err);
        }
    }
}

}  // namespace updagg

using namespace updagg;

struct GpuUpdAgg : OpBase {
    AmdUpdatingConfig cfg;
    AggSpec agg;
    UStore store;
    uint32_t cur_epoch;
    int64_t *d_out[UAGG_MAX_SW + AMD_MAX_AGGS + 4];
    unsigned long long *d_n_out;
    Staging stg;
    int n_in_cols, out_cols, drain0_cols, drain1_cols;
    int64_t out_cap;
    int has_ord;                /* config has MEDIAN / MIN_RETRACT / MAX_RETRACT */
    OrdEnt *d_arena;            /* [pool_cap] wide-chain scratch (has_ord) */
    unsigned long long *d_arena_cur;
    int f64;                    /* some value column is f64: the *_f64 kernels */
    /* null semantics (cfg.null_semantics == 1) only */
    int ns;
    uint32_t *d_lastv;          /* [C+1] last-emitted validity mask */
    uint32_t *d_vmask;          /* [out_cap] per emitted row */
    uint64_t *d_bm;             /* [n_aggs * bm_words] packed output bitmaps */
    int64_t bm_words;
    unsigned int *d_nullcols;
    Staging stg_v;              /* input bitmap staging, per value column,
                                   stg.cap / 64 words */
};

static bool ua_is_ord(int op) {
    return op == AMD_AGG_MEDIAN || op == AMD_AGG_MIN_RETRACT ||
           op == AMD_AGG_MAX_RETRACT;
}

API void *arroyo_amd_updagg_create(const AmdUpdatingConfig *cfg) {
    if (!cfg || cfg->n_keys < 0 || cfg->n_keys > 1 || cfg->n_value_cols < 0 ||
        cfg->n_value_cols > 8 || cfg->n_aggs < 1 ||
        cfg->n_aggs > AMD_MAX_AGGS) {
        snprintf(g_create_err, sizeof g_create_err, "invalid updagg config");
        return nullptr;
    }
    int has_ord = 0;
    for (int i = 0; i < cfg->n_aggs; i++) {
        int op = cfg->agg_ops[i];
        if (op < AMD_AGG_COUNT || op > AMD_AGG_MAX_RETRACT) {
            snprintf(g_create_err, sizeof g_create_err,
                     "invalid updagg config: unknown aggregate op %d", op);
            return nullptr;
        }
        if (ua_is_ord(op)) {
            if (cfg->agg_col[i] < 0 || cfg->agg_col[i] >= cfg->n_value_cols) {
                snprintf(g_create_err, sizeof g_create_err,
                         "invalid updagg config: aggregate op %d needs a "
                         "value column", op);
                return nullptr;
            }
            has_ord = 1;
        }
    }
    if (cfg->null_semantics != 0 && cfg->null_semantics != 1) {
        snprintf(g_create_err, sizeof g_create_err,
                 "invalid updagg config: null_semantics %d (0 or 1)",
                 cfg->null_semantics);
        return nullptr;
    }
    uint32_t f64m = 0;
    for (int c = 0; c < 8; c++) {
        int f = cfg->val_is_f64[c];
        if (f != 0 && f != 1) {
            snprintf(g_create_err, sizeof g_create_err,
                     "invalid updagg config: val_is_f64[%d] = %d (0 or 1)",
                     c, f);
            return nullptr;
        }
        if (f && c >= cfg->n_value_cols) {
            snprintf(g_create_err, sizeof g_create_err,
                     "invalid updagg config: val_is_f64[%d] set, but there "
                     "are %d value columns", c, cfg->n_value_cols);
            return nullptr;
        }
        if (f) f64m |= 1u << c;
    }
    for (int i = 0; i < cfg->n_aggs; i++) {
        int op = cfg->agg_ops[i], col = cfg->agg_col[i];
        if ((op == AMD_AGG_BIT_AND || op == AMD_AGG_BIT_OR ||
             op == AMD_AGG_BIT_XOR) &&
            col >= 0 && col < 8 && ((f64m >> col) & 1)) {
            snprintf(g_create_err, sizeof g_create_err,
                     "invalid updagg config: bitwise aggregate op %d over "
                     "f64 value column %d", op, col);
            return nullptr;
        }
    }
    GpuUpdAgg *o = new GpuUpdAgg();
    o->cfg = *cfg;
    o->has_ord = has_ord;
    o->ns = cfg->null_semantics;
    o->f64 = f64m != 0;
    o->agg.f64m = f64m;
    o->agg.n_aggs = cfg->n_aggs;
    o->agg.SW = 0;
    for (int i = 0; i < cfg->n_aggs; i++) {
        o->agg.op[i] = cfg->agg_ops[i];
        o->agg.col[i] = cfg->agg_col[i];
        o->agg.col2[i] = cfg->agg_col2[i];
        o->agg.soff[i] = o->agg.SW;
        o->agg.SW += ua_width(cfg->agg_ops[i], o->ns);
    }
    if (o->agg.SW > UAGG_MAX_SW) {
        snprintf(g_create_err, sizeof g_create_err,
                 "aggregate state too wide (%d words > %d)", o->agg.SW,
                 UAGG_MAX_SW);
        delete o;
        return nullptr;
    }
    o->store.C = 1u << (cfg->log2_capacity ? cfg->log2_capacity : 16);
    o->store.pool_cap = 1ll << (cfg->log2_nodes ? cfg->log2_nodes : 20);
    o->out_cap = 1ll << (cfg->log2_out_cap ? cfg->log2_out_cap : 20);
    o->n_in_cols = cfg->n_keys + cfg->n_value_cols + 1;
    o->out_cols = cfg->n_keys + cfg->n_aggs + 1;
    o->drain0_cols = cfg->n_keys + 1 + o->agg.SW + 1 + cfg->n_aggs +
                     (o->ns ? 1 : 0);
    o->drain1_cols = cfg->n_keys + 3;
    o->cur_epoch = 1;
    if (hipSetDevice(cfg->device) != hipSuccess) {
        snprintf(g_create_err, sizeof g_create_err,
                 "hipSetDevice(%d) failed: no HIP device (no CPU fallback)",
                 cfg->device);
        delete o;
        return nullptr;
    }
    size_t C1 = (size_t)o->store.C + 1;
    size_t na = cfg->n_aggs;
    OP_ALLOC(o, o->store.keys, C1 * 8, 0xFF);
    OP_ALLOC(o, o->store.epoch, C1 * 4, 0);
    OP_ALLOC(o, o->store.rows, C1 * 8, 0);
    /* every state's identity is the zero pattern (enc_min/enc_max map the
     * MIN/MAX identities to 0; f64 sums start at +0.0 = zero bits; bit
     * counters at 0), so a plain memset initializes the plane */
    OP_ALLOC(o, o->store.st, C1 * (size_t)o->agg.SW * 8, 0);
    OP_ALLOC(o, o->store.last, C1 * na * 8);
    OP_ALLOC(o, o->store.emitted, C1 * 4, 0);
    OP_ALLOC(o, o->store.head, C1 * 8 * 4, 0xFF);
    OP_ALLOC(o, o->store.pool, (size_t)o->store.pool_cap * sizeof(Node));
    OP_ALLOC(o, o->store.pool_cur, 8, 0);
    if (o->has_ord) {
        /* no reset needed between flushes: k_updagg_ordstat writes ord for
         * exactly the (slot, agg) pairs k_updagg_flush then reads */
        OP_ALLOC(o, o->store.ord, C1 * na * 8);
        OP_ALLOC(o, o->d_arena, (size_t)o->store.pool_cap * sizeof(OrdEnt));
        OP_ALLOC(o, o->d_arena_cur, 8);
    }
    int max_out = o->drain0_cols;
    if (o->drain1_cols > max_out) max_out = o->drain1_cols;
    if (o->out_cols > max_out) max_out = o->out_cols;
    for (int i = 0; i < max_out; i++)
        OP_ALLOC(o, o->d_out[i], (size_t)o->out_cap * 8);
    OP_ALLOC(o, o->d_n_out, 8);
    OP_ALLOC(o, o->d_err, 4, 0);
    if (o->ns) {
        o->bm_words = o->out_cap / 64 + 1;
        OP_ALLOC(o, o->d_lastv, C1 * 4, 0);
        OP_ALLOC(o, o->d_vmask, (size_t)o->out_cap * 4);
        OP_ALLOC(o, o->d_bm, na * (size_t)o->bm_words * 8);
        OP_ALLOC(o, o->d_nullcols, 4);
    }
    OP_TRY(o, "hipStreamCreate", o->stream_create(&o->stream));
    OP_TRY_MSG(o, "updagg staging alloc failed",
               o->stg.alloc(o, o->n_in_cols, 1 << 20));
    if (o->ns)
        OP_TRY_MSG(o, "updagg validity staging alloc failed",
                   o->stg_v.alloc(o, cfg->n_value_cols, o->stg.cap / 64));
    return o;
}

API const char *arroyo_amd_updagg_last_error(void *h) {
    return h ? ((GpuUpdAgg *)h)->err_msg : g_create_err;
}

static const char *ua_err_msg(int e) {
    return e == UERR_TABLE_FULL ? "key table full; raise log2_capacity"
           : e == UERR_POOL_FULL
               ? "distinct-value node pool full; raise log2_nodes"
           : e == UERR_OUT_CAP ? "output buffer full; raise log2_out_cap"
           : e == UERR_RETRACT
               ? "MIN/MAX do not support retraction (append-only here)"
           : e == UERR_ORD_ROWS
               ? "ordered aggregate: retraction without a matching append"
           : e == UERR_ORD_CHAIN
               ? "ordered aggregate: value chain exceeds the node pool"
               : "device error";
}

static int ua_check_cols(GpuUpdAgg *o, int32_t n_cols) {
    if (n_cols == o->n_in_cols) return 0;
    snprintf(o->err_msg, sizeof o->err_msg, "expected %d cols, got %d",
             o->n_in_cols, n_cols);
    return 1;
}

static void ua_fill_update_args(GpuUpdAgg *o, UpdateArgs *A, int64_t n_rows) {
    A->n_keys = o->cfg.n_keys;
    A->n_vals = o->cfg.n_value_cols;
    A->n_rows = n_rows;
    A->store = o->store;
    A->agg = o->agg;
    A->cur_epoch = o->cur_epoch;
    A->err = o->d_err;
}

/* the update kernel of this operator's (null_semantics, f64) pair */
static void ua_launch_update(GpuUpdAgg *o, const UpdateArgsN &N,
                             int64_t n_rows) {
    dim3 grid(grid_for(n_rows, 2048)), block(256);
    if (o->ns && o->f64)
        hipLaunchKernelGGL(k_updagg_update_nullable_f64, grid, block, 0,
                           o->stream, N);
    else if (o->ns)
        hipLaunchKernelGGL(k_updagg_update_nullable, grid, block, 0,
                           o->stream, N);
    else if (o->f64)
        hipLaunchKernelGGL(k_updagg_update_f64, grid, block, 0, o->stream,
                           N.A);
    else
        hipLaunchKernelGGL(k_updagg_update, grid, block, 0, o->stream, N.A);
}

/* shared argument checks of the nullable entry points */
static int ua_check_nullable(GpuUpdAgg *o, const uint8_t *const *validity,
                             int32_t n_cols) {
    if (!o->ns) {
        snprintf(o->err_msg, sizeof o->err_msg,
                 "process_batch_nullable needs a handle created with "
                 "null_semantics = 1");
        return 1;
    }
    if (ua_check_cols(o, n_cols)) return 1;
    if (validity) {
        if (o->cfg.n_keys && validity[0]) {
            snprintf(o->err_msg, sizeof o->err_msg,
                     "validity bitmap on the key column: NULL group keys "
                     "are not supported");
            return 1;
        }
        if (validity[n_cols - 1]) {
            snprintf(o->err_msg, sizeof o->err_msg,
                     "validity bitmap on the is_retract column: it is "
                     "non-nullable");
            return 1;
        }
    }
    return 0;
}

/* host ingest; validity == nullptr (or an entry of it) = all valid.  Chunks
 * are stg.cap = 2^20 rows, so a chunk starts on a bitmap byte boundary. */
static int ua_process_host(GpuUpdAgg *o, const int64_t *const *cols,
                           const uint8_t *const *validity, int32_t n_cols,
                           int64_t n_rows) {
    int64_t done = 0;
    while (done < n_rows) {
        int64_t take = n_rows - done;
        if (take > o->stg.cap) take = o->stg.cap;
        UpdateArgsN N = {};
        UpdateArgs &A = N.A;
        if (o->stg.stage_chunk(o, cols, n_cols, done, take, A.cols)) return 1;
        for (int v = 0; validity && v < o->cfg.n_value_cols; v++) {
            const uint8_t *bm = validity[o->cfg.n_keys + v];
            if (!bm) continue;
            size_t nbytes = (size_t)((take + 7) / 8);
            size_t nwords = (size_t)((take + 63) / 64);
            o->stg_v.h[v][nwords - 1] = 0;   /* pad the last word */
            memcpy(o->stg_v.h[v], bm + done / 8, nbytes);
            HIP_CHECK(o, hipMemcpyAsync(o->stg_v.d[v], o->stg_v.h[v],
                                        nwords * 8, hipMemcpyHostToDevice,
                                        o->stream));
            N.valid[v] = (const uint64_t *)o->stg_v.d[v];
        }
        ua_fill_update_args(o, &A, take);
        ua_launch_update(o, N, take);
        HIP_CHECK(o, hipGetLastError());
        HIP_CHECK(o, hipStreamSynchronize(o->stream));
        done += take;
    }
    return 0;
}

static int ua_process_device(GpuUpdAgg *o, const int64_t *const *dcols,
                             const uint8_t *const *dvalidity, int32_t n_cols,
                             int64_t n_rows) {
    UpdateArgsN N = {};
    UpdateArgs &A = N.A;
    for (int c = 0; c < n_cols; c++) A.cols[c] = dcols[c];
    for (int v = 0; dvalidity && v < o->cfg.n_value_cols; v++) {
        const uint8_t *bm = dvalidity[o->cfg.n_keys + v];
        if ((uintptr_t)bm & 7) {
            snprintf(o->err_msg, sizeof o->err_msg,
                     "device validity bitmap of column %d is not 8-byte "
                     "aligned", o->cfg.n_keys + v);
            return 1;
        }
        N.valid[v] = (const uint64_t *)bm;
    }
    ua_fill_update_args(o, &A, n_rows);
    ua_launch_update(o, N, n_rows);
    HIP_CHECK(o, hipGetLastError());
    return 0;
}

API int arroyo_amd_updagg_process_batch(void *h, const int64_t *const *cols,
                                        int32_t n_cols, int64_t n_rows) {
    GpuUpdAgg *o = (GpuUpdAgg *)h;
    if (ua_check_cols(o, n_cols)) return 1;
    return ua_process_host(o, cols, nullptr, n_cols, n_rows);
}

API int arroyo_amd_updagg_process_batch_device(void *h,
                                               const int64_t *const *dcols,
                                               int32_t n_cols,
                                               int64_t n_rows) {
    GpuUpdAgg *o = (GpuUpdAgg *)h;
    if (ua_check_cols(o, n_cols)) return 1;
    return ua_process_device(o, dcols, nullptr, n_cols, n_rows);
}

API int arroyo_amd_updagg_process_batch_nullable(
    void *h, const int64_t *const *cols, const uint8_t *const *validity,
    int32_t n_cols, int64_t n_rows) {
    GpuUpdAgg *o = (GpuUpdAgg *)h;
    if (ua_check_nullable(o, validity, n_cols)) return 1;
    return ua_process_host(o, cols, validity, n_cols, n_rows);
}

API int arroyo_amd_updagg_process_batch_nullable_device(
    void *h, const int64_t *const *dcols, const uint8_t *const *dvalidity,
    int32_t n_cols, int64_t n_rows) {
    GpuUpdAgg *o = (GpuUpdAgg *)h;
    if (ua_check_nullable(o, dvalidity, n_cols)) return 1;
    return ua_process_device(o, dcols, dvalidity, n_cols, n_rows);
}

/* null semantics: pack the emitted rows' validity masks (d_vmask) into
 * per-aggregate Arrow bitmaps on the device and attach to `out` the bitmaps
 * of the aggregate columns that hold at least one NULL.  Key and is_retract
 * columns, and fully valid aggregate columns, keep a NULL pointer.  A
 * failed allocation is an error, never an "all valid". */
static int ua_fill_validity(GpuUpdAgg *o, AmdOutBatch *out) {
    if (!o->ns) return 0;
    int64_t n = out->n_rows;
    if (out_alloc_validity(out)) {
        snprintf(o->err_msg, sizeof o->err_msg,
                 "validity bitmap table allocation failed");
        return 1;
    }
    if (n == 0) return 0;
    int na = o->cfg.n_aggs;
    HIP_CHECK(o, hipMemsetAsync(o->d_nullcols, 0, 4, o->stream));
    PackArgs P = {};
    P.vmask = o->d_vmask;
    P.n_rows = n;
    P.n_aggs = na;
    for (int a = 0; a < na; a++) P.bm[a] = o->d_bm + (size_t)a * o->bm_words;
    P.nullcols = o->d_nullcols;
    hipLaunchKernelGGL(k_updagg_pack_validity, dim3(grid_for(n, 2048)),
                       dim3(256),
                       0, o->stream, P);
    HIP_CHECK(o, hipGetLastError());
    unsigned int nullcols = 0;
    HIP_CHECK(o, hipMemcpyAsync(&nullcols, o->d_nullcols, 4,
                                hipMemcpyDeviceToHost, o->stream));
    HIP_CHECK(o, hipStreamSynchronize(o->stream));
    size_t nbytes = (size_t)((n + 7) / 8);
    for (int a = 0; a < na; a++) {
        if (!((nullcols >> a) & 1)) continue;
        uint8_t *bm = out_validity_col(out, o->cfg.n_keys + a);
        if (!bm) {
            snprintf(o->err_msg, sizeof o->err_msg,
                     "validity bitmap allocation failed (%zu bytes)", nbytes);
            return 1;
        }
        HIP_CHECK(o, hipMemcpyAsync(bm, P.bm[a], nbytes, hipMemcpyDeviceToHost,
                                    o->stream));
    }
    HIP_CHECK(o, hipStreamSynchronize(o->stream));
    return 0;
}

/* the emitted rows and their bitmaps into the allocated batch; an error
 * leaves `out` freed and zeroed */
static int ua_out_rows(GpuUpdAgg *o, AmdOutBatch *out, int64_t n) {
    /* f64 outputs, on flush and expire alike: AVG and the moment families
     * always, and the aggregates that hand an f64 argument through */
    for (int a = 0; a < o->cfg.n_aggs; a++) {
        int op = o->cfg.agg_ops[a];
        if (op == AMD_AGG_AVG ||
            (op >= AMD_AGG_STDDEV && op <= AMD_AGG_VAR_POP) ||
            (ua_is_comoment(op) && op != AMD_AGG_REGR_COUNT) ||
            ((op == AMD_AGG_SUM || op == AMD_AGG_MIN || op == AMD_AGG_MAX ||
              ua_is_ord(op)) &&
             ua_f64_col(o->agg, o->cfg.agg_col[a])))
            out->is_f64[o->cfg.n_keys + a] = 1;
    }
    if (out_copy_cols(o, out, o->d_out, n)) return 1;
    if (!ua_fill_validity(o, out)) return 0;
    out_free_host(out);
    return 1;
}

API int arroyo_amd_updagg_flush(void *h, AmdOutBatch *out) {
    GpuUpdAgg *o = (GpuUpdAgg *)h;
    if (op_check_err(o, ua_err_msg)) return 1;
    HIP_CHECK(o, hipMemsetAsync(o->d_n_out, 0, 8, o->stream));
    if (o->has_ord) {
        /* order-statistic pre-pass: one wave per 8 slots, grid-strided */
        HIP_CHECK(o, hipMemsetAsync(o->d_arena_cur, 0, 8, o->stream));
        OrdArgs R = {};
        R.store = o->store;
        R.agg = o->agg;
        R.cur_epoch = o->cur_epoch;
        R.arena = o->d_arena;
        R.arena_cur = o->d_arena_cur;
        R.arena_cap = o->store.pool_cap;
        R.err = o->d_err;
        int64_t waves = ((int64_t)o->store.C + 1 + 7) / 8;
        auto ordk = o->ns ? (o->f64 ? k_updagg_ordstat_nullable_f64
                                    : k_updagg_ordstat_nullable)
                          : (o->f64 ? k_updagg_ordstat_f64 : k_updagg_ordstat);
        hipLaunchKernelGGL(ordk, dim3(grid_for(waves * 64, 2048)),
                           dim3(64 * UORD_WAVES), 0, o->stream, R);
        HIP_CHECK(o, hipGetLastError());
    }
    FlushArgs F = {};
    F.store = o->store;
    F.agg = o->agg;
    F.cur_epoch = o->cur_epoch;
    F.n_keys = o->cfg.n_keys;
    for (int i = 0; i < o->out_cols; i++) F.out[i] = o->d_out[i];
    F.n_out = o->d_n_out;
    F.out_cap = o->out_cap;
    F.err = o->d_err;
    F.lastv = o->d_lastv;
    F.vmask = o->d_vmask;
    auto flushk = o->ns ? (o->f64 ? k_updagg_flush_nullable_f64
                                  : k_updagg_flush_nullable)
                        : (o->f64 ? k_updagg_flush_f64 : k_updagg_flush);
    hipLaunchKernelGGL(flushk, dim3(grid_for((int64_t)o->store.C + 1, 2048)),
                       dim3(256), 0, o->stream, F);
    HIP_CHECK(o, hipGetLastError());
    unsigned long long n = 0;
    HIP_CHECK(o, hipMemcpyAsync(&n, o->d_n_out, 8, hipMemcpyDeviceToHost,
                                o->stream));
    HIP_CHECK(o, hipStreamSynchronize(o->stream));
    if (op_check_err(o, ua_err_msg)) return 1;
    o->cur_epoch++;
    if (out) {
        if (op_out_alloc(o, out, (int64_t)n, o->out_cols, __func__))
            return 1;
        if (ua_out_rows(o, out, (int64_t)n)) return 1;
    }
    return 0;
}

API int arroyo_amd_updagg_expire(void *h, int64_t idle_flushes,
                                 AmdOutBatch *out) {
    GpuUpdAgg *o = (GpuUpdAgg *)h;
    if (op_check_err(o, ua_err_msg)) return 1;
    HIP_CHECK(o, hipMemsetAsync(o->d_n_out, 0, 8, o->stream));
    ExpireArgs E = {};
    E.store = o->store;
    E.agg = o->agg;
    E.cur_epoch = o->cur_epoch;
    E.idle = (uint32_t)idle_flushes;
    E.n_keys = o->cfg.n_keys;
    for (int i = 0; i < o->out_cols; i++) E.out[i] = o->d_out[i];
    E.n_out = o->d_n_out;
    E.out_cap = o->out_cap;
    E.err = o->d_err;
    E.lastv = o->d_lastv;
    E.vmask = o->d_vmask;
    hipLaunchKernelGGL(k_updagg_expire,
                       dim3(grid_for((int64_t)o->store.C + 1, 2048)),
                       dim3(256), 0,
                       o->stream, E);
    HIP_CHECK(o, hipGetLastError());
    unsigned long long n = 0;
    HIP_CHECK(o, hipMemcpyAsync(&n, o->d_n_out, 8, hipMemcpyDeviceToHost,
                                o->stream));
    HIP_CHECK(o, hipStreamSynchronize(o->stream));
    if (op_check_err(o, ua_err_msg)) return 1;
    if (out && (op_out_alloc(o, out, (int64_t)n, o->out_cols, __func__) ||
                ua_out_rows(o, out, (int64_t)n)))
        return 1;
    return 0;
}

API int arroyo_amd_updagg_checkpoint_drain(void *h, int32_t which,
                                           AmdOutBatch *out) {
    GpuUpdAgg *o = (GpuUpdAgg *)h;
    if (op_check_err(o, ua_err_msg)) return 1;
    int ncols = which == 0 ? o->drain0_cols : o->drain1_cols;
    HIP_CHECK(o, hipMemsetAsync(o->d_n_out, 0, 8, o->stream));
    UDrainArgs D = {};
    D.store = o->store;
    D.agg = o->agg;
    D.n_keys = o->cfg.n_keys;
    D.which = which;
    for (int i = 0; i < ncols; i++) D.out[i] = o->d_out[i];
    D.n_out = o->d_n_out;
    D.out_cap = o->out_cap;
    D.err = o->d_err;
    D.lastv = o->d_lastv;
    hipLaunchKernelGGL(k_updagg_drain,
                       dim3(grid_for((int64_t)o->store.C + 1, 2048)),
                       dim3(256), 0,
                       o->stream, D);
    HIP_CHECK(o, hipGetLastError());
    unsigned long long n = 0;
    HIP_CHECK(o, hipMemcpyAsync(&n, o->d_n_out, 8, hipMemcpyDeviceToHost,
                                o->stream));
    HIP_CHECK(o, hipStreamSynchronize(o->stream));
    if (op_check_err(o, ua_err_msg)) return 1;
    return op_out_alloc(o, out, (int64_t)n, ncols, __func__) ||
           out_copy_cols(o, out, o->d_out, (int64_t)n);
}

API int arroyo_amd_updagg_restore(void *h, int32_t which,
                                  const int64_t *const *cols, int32_t n_cols,
                                  int64_t n_rows) {
    GpuUpdAgg *o = (GpuUpdAgg *)h;
    int want = which == 0 ? o->drain0_cols : o->drain1_cols;
    if (n_cols != want) {
        snprintf(o->err_msg, sizeof o->err_msg,
                 "restore(%d) expects %d cols, got %d", which, want, n_cols);
        return 1;
    }
    int64_t done = 0;
    while (done < n_rows) {
        int64_t take = n_rows - done;
        if (take > o->stg.cap) take = o->stg.cap;
        URestoreArgs R = {};
        /* restore columns can exceed the input staging set: ad hoc device
         * buffers for this control-rate path, freed at the end of the
         * iteration */
        DevScratch tmp;
        for (int c = 0; c < n_cols; c++) {
            int64_t *d;
            HIP_CHECK(o, tmp.upload(d, cols[c] + done, (size_t)take));
            R.cols[c] = d;
        }
        R.n_cols = n_cols;
        R.n_rows = take;
        R.store = o->store;
        R.agg = o->agg;
        R.n_keys = o->cfg.n_keys;
        R.which = which;
        R.err = o->d_err;
        R.lastv = o->d_lastv;
        hipLaunchKernelGGL(k_updagg_restore, dim3(grid_for(take, 2048)),
                           dim3(256),
                           0, o->stream, R);
        HIP_CHECK(o, hipGetLastError());
        HIP_CHECK(o, hipStreamSynchronize(o->stream));
        done += take;
    }
    return op_check_err(o, ua_err_msg);
}

API void arroyo_amd_updagg_destroy(void *h) {
    delete (GpuUpdAgg *)h;   /* ~OpBase drains the stream first */
}
