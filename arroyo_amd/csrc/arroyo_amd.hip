/* arroyo-amd: MI355X-native (gfx950) execution path for Arroyo's
 * windowed-aggregate operator hot path.
 *
 * This is the PRODUCT library behind the C ABI declared in
 * include/arroyo_amd.h.  It replaces, behind the reference's own operator
 * boundary (ArrowOperator, crates/arroyo-operator/src/operator.rs:1144-1257),
 * the per-batch work of:
 *   - SlidingAggregatingWindowFunc
 *     (crates/arroyo-worker/src/arrow/sliding_aggregating_window.rs)
 *   - TumblingAggregatingWindowFunc
 *     (crates/arroyo-worker/src/arrow/tumbling_aggregating_window.rs)
 * i.e. SURVEY.md SS2 kernel rows K1 (date_bin binning), K2 (sort/partition by
 * bin), K3 (partial hash group-by), K4 (partial-merge final aggregate),
 * K5 (final projection), K9 (watermark eviction).
 *
 * MI355X-first design (NOT a translation of the reference's
 * sort+take+DataFusion-stream structure):
 *   - Window state is a device-resident ring of per-pane open-addressing
 *     hash tables in HBM.  One fused update kernel replaces K1+K2+K3:
 *     per row it computes the bin (ts - ts % slide), applies the late-data
 *     drop, claims the pane's ring slot, and atomically updates the
 *     (key -> partial state) entry.  The reference's comparison sort +
 *     full-batch `take` copy exists only to feed per-bin DataFusion streams
 *     and is not needed on a GPU: scatter-by-hash IS the grouping.
 *   - Aggregate states are encoded so that the additive/max identity is the
 *     zero bit pattern (MIN/MAX order-preserving transforms into u64-max
 *     domain), so pane retirement (K9) is hipMemsetAsync and inserts need no
 *     init handshake: any lane may atomically fold its row into a slot the
 *     moment the key CAS lands.
 *   - Watermark advance (K4+K5): the fused hash-aligned kernel
 *     k_merge_fused (one workgroup per home-slot range, LDS dedup across
 *     panes, direct emission — no merge table, no state atomics) for
 *     narrow aggregate sets; the legacy merge-table k_merge + k_compact
 *     pair for wide sets and checkpoint drains.  Outputs stay
 *     device-resident unless emit_to_host is set.
 *   - The watermark/firing state machine stays on the host (it is
 *     control-rate), replicated statement-for-statement from the reference
 *     (see host section below); the only per-watermark device traffic is a
 *     ring-tag snapshot + the merge/compact launches.
 *
 * Semantics are pinned bit-for-bit against oracle/arroyo_oracle.c (itself
 * pinned against the reference's golden vectors) by tests/test_gpu_parity.py.
 */
#include <map>
#include <set>
#include <string>

#include "op_common.h"

/* ------------------------------------------------------------------ */
/* device-side layout                                                  */

#define ERR_RING_CONFLICT 2

/* per-word merge ops over the encoded state domain */
enum WordOp { W_ADD_I64 = 0, W_MAX_U64 = 1, W_ADD_F64 = 2, W_NONE = 3 };

struct DeviceRing {
    int64_t  *keys;      /* [R][C] */
    uint64_t *state;     /* [R][C][n_aggs][2] encoded */
    uint64_t *tag;       /* [R] bin nanos or EMPTY_TAG */
    /* special entry per pane for an actual key == EMPTY_KEY */
    uint32_t *spec_used; /* [R] */
    uint64_t *spec_state;/* [R][n_aggs][2] */
    int      *err;
    uint64_t *min_bin;   /* running min of non-late bins (state machine) */
    uint32_t  C;         /* slots per pane, power of two */
    uint32_t  R;         /* panes in ring, power of two */
};

struct AggSpec {
    int32_t n_aggs;
    int32_t op[AMD_MAX_AGGS];
    int32_t col[AMD_MAX_AGGS];
    int32_t isf[AMD_MAX_AGGS];  /* value column is f64 (bit pattern in the
                                   i64 plane); COUNT/AVG-count unaffected */
};

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

/* the f64 encodings (enc_minf .. dec_maxf) are op_common.h's, shared with
 * the updating aggregate */

/* encode one raw (i64 or f64-bits) value into the op's state domain */
__host__ __device__ inline uint64_t enc_word(int op, int isf, int64_t raw) {
    switch (op) {
    case AMD_AGG_MIN: return isf ? enc_minf(raw) : enc_min(raw);
    case AMD_AGG_MAX: return isf ? enc_maxf(raw) : enc_max(raw);
    default: return (uint64_t)raw;    /* COUNT/SUM/AVG words are raw */
    }
}

/* decode one state word back to the raw value domain */
__host__ __device__ inline int64_t dec_word(int op, int isf, uint64_t e) {
    switch (op) {
    case AMD_AGG_MIN: return isf ? dec_minf(e) : dec_min(e);
    case AMD_AGG_MAX: return isf ? dec_maxf(e) : dec_max(e);
    default: return (int64_t)e;
    }
}

/* floor-divide t by slide via the precomputed reciprocal; exact for all
 * t < 2^64 (q from mulhi is in {q*, q*-1}; one fixup resolves it). */
__device__ inline uint64_t div_slide(uint64_t t, uint64_t slide,
                                     uint64_t inv) {
    uint64_t q = __umul64hi(t, inv);
    if (t - q * slide >= slide) q++;
    return q;
}

/* fold one input row into an encoded state vector via atomics */
__device__ inline void atomic_update(uint64_t *st, const AggSpec a,
                                     const int64_t *const *vcols, int64_t r) {
    for (int i = 0; i < a.n_aggs; i++) {
        uint64_t *w = st + 2 * i;
        switch (a.op[i]) {
        case AMD_AGG_COUNT:
            atomicAdd((unsigned long long *)w, 1ULL);
            break;
        case AMD_AGG_SUM:
            if (a.isf[i]) {
                int64_t b = vcols[a.col[i]][r];
                double v;
                memcpy(&v, &b, 8);
                atomicAdd((double *)w, v);
            } else {
                atomicAdd((unsigned long long *)w,
                          (unsigned long long)vcols[a.col[i]][r]);
            }
            break;
        case AMD_AGG_MIN:
        case AMD_AGG_MAX:
            atomicMax((unsigned long long *)w,
                      (unsigned long long)enc_word(a.op[i], a.isf[i],
                                                   vcols[a.col[i]][r]));
            break;
        case AMD_AGG_AVG:
            atomicAdd((unsigned long long *)w, 1ULL);
            if (a.isf[i]) {
                int64_t b = vcols[a.col[i]][r];
                double v;
                memcpy(&v, &b, 8);
                atomicAdd((double *)(w + 1), v);
            } else {
                atomicAdd((double *)(w + 1), (double)vcols[a.col[i]][r]);
            }
            break;
        }
    }
}

/* merge one encoded state vector into another via atomics */
__device__ inline void atomic_merge(uint64_t *dst, const uint64_t *src,
                                    const AggSpec a) {
    for (int i = 0; i < a.n_aggs; i++) {
        switch (a.op[i]) {
        case AMD_AGG_COUNT:
            atomicAdd((unsigned long long *)(dst + 2 * i),
                      (unsigned long long)src[2 * i]);
            break;
        case AMD_AGG_SUM:
            if (a.isf[i])
                atomicAdd((double *)(dst + 2 * i),
                          *(const double *)(src + 2 * i));
            else
                atomicAdd((unsigned long long *)(dst + 2 * i),
                          (unsigned long long)src[2 * i]);
            break;
        case AMD_AGG_MIN:
        case AMD_AGG_MAX:
            atomicMax((unsigned long long *)(dst + 2 * i),
                      (unsigned long long)src[2 * i]);
            break;
        case AMD_AGG_AVG:
            atomicAdd((unsigned long long *)(dst + 2 * i),
                      (unsigned long long)src[2 * i]);
            atomicAdd((double *)(dst + 2 * i + 1),
                      *(const double *)(src + 2 * i + 1));
            break;
        }
    }
}

/* claim a pane's ring slot for `bin`; wave-cooperative callers dedup first.
 * The volatile re-read (L2, bypassing a possibly-stale L1 line) keeps the
 * CAS storm on a freshly-opened bin to the waves in flight at that moment. */
__device__ inline void claim_tag(uint64_t *tp, uint64_t bin, int *err) {
    uint64_t tag = *(volatile unsigned long long *)tp;
    if (tag == bin) return;
    uint64_t old = atomicCAS((unsigned long long *)tp,
                             (unsigned long long)EMPTY_TAG,
                             (unsigned long long)bin);
    if (old != EMPTY_TAG && old != bin) *err = ERR_RING_CONFLICT;
}

/* wave-level tag protocol: rows in a wave are usually consecutive and share
 * one bin, so one leader lane claims for everyone. */
__device__ inline void claim_tag_wave(uint64_t *tags, uint32_t p, uint64_t bin,
                                      uint64_t cached_tag, int *err) {
    if (cached_tag == bin) return;
    unsigned long long act = __ballot(1);
    int leader = (int)(__ffsll((long long)act) - 1);
    uint64_t b0 = (uint64_t)__shfl((long long)bin, leader, 64);
    if (__all(bin == b0)) {
        if ((int)(threadIdx.x & 63) == leader) claim_tag(&tags[p], bin, err);
    } else {
        claim_tag(&tags[p], bin, err);
    }
}

/* ------------------------------------------------------------------ */
/* K1+K2+K3 fused: bin, late-drop, pane-claim, hash-aggregate update.  */

struct UpdateArgs {
    const int64_t *key_col;   /* null when unkeyed */
    const int64_t *ts_col;
    const int64_t *vcols[4];
    int64_t  n_rows;
    uint64_t slide;
    uint64_t slide_inv;  /* floor(2^64 / slide): q = mulhi(t, inv) (+fixup)
                            replaces the ~100-cycle software u64 modulo */
    uint64_t wm_bin;     /* late-drop cutoff bin; 0 if no watermark yet */
    int      has_wm;
    uint64_t ts_offset;  /* added to ts (bench ring replay); 0 otherwise */
    DeviceRing ring;
    AggSpec agg;
};

__device__ inline void fold_min_bin(uint64_t local_min, uint64_t *min_bin) {
    /* wavefront reduction, then an atomic ONLY if we would improve the
     * current value: same-address atomics serialize at the L2 bank (~one
     * per few ns), so an unconditional per-wave atomicMin alone was costing
     * ~12 ns x waves per launch.  The L1-bypassing volatile read may be a
     * touch stale, which only costs a rare extra atomic. */
    for (int off = 32; off; off >>= 1) {
        uint64_t v = (uint64_t)__shfl_down((long long)local_min, off, 64);
        if (v < local_min) local_min = v;
    }
    if ((threadIdx.x & 63) == 0 && local_min != ~0ULL) {
        uint64_t cur = *(volatile unsigned long long *)min_bin;
        if (local_min < cur)
            atomicMin((unsigned long long *)min_bin,
                      (unsigned long long)local_min);
    }
}

/* pure streaming-read calibration kernel: 16 B/lane vector loads of both
 * columns, LDS-reduced to one atomic per workgroup — the ceiling any
 * update-kernel variant can reach. n must be even (rows; reads n/2 pairs). */
__global__ void __launch_bounds__(256)
k_stream_sum(const ulonglong2 *a, const ulonglong2 *b, int64_t n2,
             unsigned long long *out) {
    __shared__ unsigned long long red[4];
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    uint64_t acc = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n2;
         i += stride) {
        ulonglong2 va = a[i], vb = b[i];
        acc += va.x + va.y + vb.x + vb.y;
    }
    for (int off = 32; off; off >>= 1)
        acc += (uint64_t)__shfl_down((long long)acc, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0;
        for (unsigned w = 0; w < blockDim.x / 64; w++) t += red[w];
        atomicAdd(out, t);
    }
}

/* LDS-staged variant: each workgroup pre-aggregates its rows into an LDS
 * table (cutting global atomic traffic on hot keys -- nexmark sends ~50% of
 * bids to one auction), then flushes distinct (pane,key) entries to the
 * ring.  Entries evicted on LDS collision fall through to global atomics. */
#define LDS_SLOTS 1024   /* x (8B key + 4B pane + n_aggs*16B) */

#define PANE_UNSET 0xFFFFFFFFu

/* per-row body shared by the scalar and vectorized LDS kernels.
 * COUNT_ONLY specializes the hot q5 shape (single COUNT(*)) away from the
 * aggregate-spec loop; last_key/last_slot cache skips hash+probe when
 * consecutive rows repeat a key (the nexmark hot auction makes runs
 * common). */
template <int SLOTS, bool COUNT_ONLY>
__device__ inline void lds_update_row(const UpdateArgs &A, int64_t *ls_key,
                                      uint32_t *ls_pane, uint64_t *ls_st,
                                      int64_t row, uint64_t traw, int64_t key,
                                      uint64_t &local_min,
                                      uint64_t &last_bin, int64_t &last_key,
                                      uint32_t &last_slot) {
    const int na = A.agg.n_aggs;
    const int64_t *const *vc = A.vcols;
    uint64_t t = traw + A.ts_offset;
    uint64_t q = div_slide(t, A.slide, A.slide_inv);
    uint64_t bin = q * A.slide;
    if (A.has_wm && bin < A.wm_bin) return;
    if (bin < local_min) local_min = bin;
    uint32_t p = (uint32_t)(q & (A.ring.R - 1));
    /* register-cached bin: the tag claim (and its global tag read) runs
     * once per thread per bin transition, not once per row */
    if (bin != last_bin) {
        claim_tag_wave(A.ring.tag, p, bin, EMPTY_TAG, A.ring.err);
        last_bin = bin;
    }
    /* same (key, pane) as the previous row: reuse the cached LDS slot */
    if (key == last_key && last_slot != PANE_UNSET &&
        ls_pane[last_slot] == p) {
        if (COUNT_ONLY) {
            atomicAdd((unsigned long long *)
                          (ls_st + (size_t)last_slot * 2), 1ULL);
            return;
        }
    }
    /* try the LDS table first, fall through to global */
    bool done = false;
    if (key != EMPTY_KEY) {
        uint32_t h = (uint32_t)hash64((uint64_t)key * 0x9e37u + p) &
                     (SLOTS - 1);
        for (int pr = 0; pr < 4 && !done; pr++) {
            uint32_t s = (h + pr) & (SLOTS - 1);
            int64_t k = ls_key[s];
            bool claimed = false;
            if (k == EMPTY_KEY) {
                int64_t old = (int64_t)atomicCAS(
                    (unsigned long long *)&ls_key[s],
                    (unsigned long long)EMPTY_KEY, (unsigned long long)key);
                if (old == EMPTY_KEY) {
                    ls_pane[s] = p;
                    k = key;
                    claimed = true;
                }
                else k = old;
            }
            /* ls_pane still PANE_UNSET means another thread's claim is not
             * fully visible yet: fall through to the global path rather
             * than aggregating into an unknown pane */
            if (k == key && (claimed || ls_pane[s] == p)) {
                uint64_t *st = ls_st + (size_t)s * na * 2;
                if (COUNT_ONLY) {
                    atomicAdd((unsigned long long *)st, 1ULL);
                    last_key = key;
                    last_slot = s;
                    done = true;
                    break;
                }
                atomic_update(st, A.agg, vc, row);
                done = true;
            }
        }
    }
    if (!done) {
        uint64_t *st;
        if (key == EMPTY_KEY) {
            atomicExch(&A.ring.spec_used[p], 1u);
            st = A.ring.spec_state + (size_t)p * na * 2;
        } else {
            int64_t *keys = A.ring.keys + (size_t)p * A.ring.C;
            int64_t s = table_upsert(keys, A.ring.C, key, A.ring.err);
            if (s < 0) return;
            st = A.ring.state + ((size_t)p * A.ring.C + (size_t)s) * na * 2;
        }
        atomic_update(st, A.agg, vc, row);
    }
}

template <int SLOTS>
__device__ inline void lds_flush(const UpdateArgs &A, int64_t *ls_key,
                                 uint32_t *ls_pane, uint64_t *ls_st) {
    const int na = A.agg.n_aggs;
    for (int s = threadIdx.x; s < SLOTS; s += blockDim.x) {
        int64_t key = ls_key[s];
        if (key == EMPTY_KEY) continue;
        uint32_t p = ls_pane[s];
        int64_t *keys = A.ring.keys + (size_t)p * A.ring.C;
        int64_t slot = table_upsert(keys, A.ring.C, key, A.ring.err);
        if (slot < 0) continue;
        atomic_merge(A.ring.state +
                         ((size_t)p * A.ring.C + (size_t)slot) * na * 2,
                     ls_st + (size_t)s * na * 2, A.agg);
    }
}

template <int SLOTS>
__device__ inline void lds_init(const UpdateArgs &A, int64_t *ls_key,
                                uint32_t *ls_pane, uint64_t *ls_st) {
    const int na = A.agg.n_aggs;
    for (int i = threadIdx.x; i < SLOTS; i += blockDim.x) {
        ls_key[i] = EMPTY_KEY;
        ls_pane[i] = PANE_UNSET;   /* sentinel: claim not yet visible */
        for (int w = 0; w < na * 2; w++) ls_st[(size_t)i * na * 2 + w] = 0;
    }
    __syncthreads();
}

__global__ void __launch_bounds__(256)
k_update_lds(UpdateArgs A) {
    __shared__ int64_t  ls_key[LDS_SLOTS];
    __shared__ uint32_t ls_pane[LDS_SLOTS];
    extern __shared__ uint64_t ls_st[];   /* [LDS_SLOTS][n_aggs][2] */
    lds_init<LDS_SLOTS>(A, ls_key, ls_pane, ls_st);
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    uint64_t local_min = ~0ULL, last_bin = EMPTY_TAG;
    int64_t last_key = EMPTY_KEY;
    uint32_t last_slot = PANE_UNSET;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         i < A.n_rows; i += stride)
        lds_update_row<LDS_SLOTS, false>(A, ls_key, ls_pane, ls_st, i,
                                         (uint64_t)A.ts_col[i],
                                         A.key_col ? A.key_col[i] : 0,
                                         local_min, last_bin, last_key,
                                         last_slot);
    fold_min_bin(local_min, A.ring.min_bin);
    __syncthreads();
    lds_flush<LDS_SLOTS>(A, ls_key, ls_pane, ls_st);
}

/* vectorized variant: 16 B/lane loads of the ts (and key) columns, two rows
 * per thread per iteration -- requires 16 B-aligned column pointers (host
 * checks).  Fewer, fatter waves: wave-dispatch cost was measurable at one
 * 8 B load per thread. */
template <int SLOTS, bool COUNT_ONLY>
__global__ void __launch_bounds__(256)
k_update_lds_vec(UpdateArgs A) {
    __shared__ int64_t  ls_key[SLOTS];
    __shared__ uint32_t ls_pane[SLOTS];
    extern __shared__ uint64_t ls_st[];
    lds_init<SLOTS>(A, ls_key, ls_pane, ls_st);
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    uint64_t local_min = ~0ULL, last_bin = EMPTY_TAG;
    int64_t last_key = EMPTY_KEY;
    uint32_t last_slot = PANE_UNSET;
    int64_t n2 = A.n_rows >> 1;
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < n2;
         v += stride) {
        ulonglong2 tsv = ((const ulonglong2 *)A.ts_col)[v];
        int64_t k0 = 0, k1 = 0;
        if (A.key_col) {
            ulonglong2 kv = ((const ulonglong2 *)A.key_col)[v];
            k0 = (int64_t)kv.x;
            k1 = (int64_t)kv.y;
        }
        lds_update_row<SLOTS, COUNT_ONLY>(
            A, ls_key, ls_pane, ls_st, 2 * v, tsv.x, k0, local_min,
            last_bin, last_key, last_slot);
        lds_update_row<SLOTS, COUNT_ONLY>(
            A, ls_key, ls_pane, ls_st, 2 * v + 1, tsv.y, k1, local_min,
            last_bin, last_key, last_slot);
    }
    if ((A.n_rows & 1) && blockIdx.x == 0 && threadIdx.x == 0)
        lds_update_row<SLOTS, COUNT_ONLY>(A, ls_key, ls_pane,
                                          ls_st, A.n_rows - 1,
                                          (uint64_t)A.ts_col[A.n_rows - 1],
                                          A.key_col ? A.key_col[A.n_rows - 1]
                                                    : 0,
                                          local_min, last_bin, last_key,
                                          last_slot);
    fold_min_bin(local_min, A.ring.min_bin);
    __syncthreads();
    lds_flush<SLOTS>(A, ls_key, ls_pane, ls_st);
}

template __global__ void k_update_lds_vec<LDS_SLOTS, false>(UpdateArgs);
template __global__ void k_update_lds_vec<LDS_SLOTS, true>(UpdateArgs);

/* ------------------------------------------------------------------ */
/* Batched-probe update kernel (UPD_BATCH, ARROYO_AMD_UPD=batch; the
 * default for the keyed single-COUNT shape before k_update_tile, which
 * reuses its row path).  Measurement drove this shape: a wave-combine
 * variant's per-row ballots made every row cost the wave max(lane
 * latencies) — the wave could not start row i+1 until the slowest cold
 * lane's global probe for row i landed (107 us vs the LDS kernel's 71 us
 * per 1.85M rows).  Here there is NO cross-lane coordination in the row
 * loop at all: each thread takes Q consecutive rows per iteration,
 * collapses sequential same-key runs (the nexmark hot key arrives in
 * runs), checks its register cache, then issues the remaining rows'
 * first probe loads back-to-back (independent -> memory-level
 * parallelism Q) before resolving any of them.  Count updates are
 * no-return atomicAdds (fire-and-forget): same-address hot-key traffic
 * queues at the memory-side cache without stalling the wave (~9 adds/us
 * needed vs the measured ~88/us single-address ceiling). */

__device__ inline uint64_t *probe_resolve(int64_t *keys, uint64_t *state,
                                          uint32_t C, int *err, int64_t key,
                                          uint64_t i, int64_t kk) {
    /* `kk` is the already-loaded key at probe position `i`; keys/state are
     * the pane's planes */
    uint64_t m = C - 1;
    uint32_t lim = C < MAX_PROBES ? C : MAX_PROBES;
    for (uint32_t probes = 0; probes < lim; probes++) {
        if (kk == key) return state + i * 2;
        if (kk == EMPTY_KEY) {
            int64_t old = (int64_t)atomicCAS((unsigned long long *)&keys[i],
                                             (unsigned long long)EMPTY_KEY,
                                             (unsigned long long)key);
            if (old == EMPTY_KEY || old == key) return state + i * 2;
        }
        i = (i + 1) & m;
        kk = keys[i];
    }
    *err = ERR_TABLE_FULL;
    return nullptr;
}

/* scalar one-row path (tail rows, misaligned columns; noinline keeps the
 * hot kernel's CFG small — an inlined copy ICEd clang-22's simplifycfg) */
__device__ __noinline__ void batch_row_scalar(const UpdateArgs &A, uint64_t traw,
                                        int64_t key, uint64_t &local_min,
                                        uint64_t &last_bin, int64_t &last_key,
                                        uint32_t &last_pane,
                                        uint64_t *&last_cnt) {
    uint64_t t = traw + A.ts_offset;
    uint64_t q = div_slide(t, A.slide, A.slide_inv);
    uint64_t bin = q * A.slide;
    if (A.has_wm && bin < A.wm_bin) return;
    if (bin < local_min) local_min = bin;
    uint32_t p = (uint32_t)(q & (A.ring.R - 1));
    if (bin != last_bin) {
        claim_tag(&A.ring.tag[p], bin, A.ring.err);
        last_bin = bin;
    }
    if (key == EMPTY_KEY) {
        atomicExch(&A.ring.spec_used[p], 1u);
        atomicAdd((unsigned long long *)(A.ring.spec_state + (size_t)p * 2),
                  1ULL);
        return;
    }
    if (key == last_key && p == last_pane && last_cnt) {
        atomicAdd((unsigned long long *)last_cnt, 1ULL);
        return;
    }
    uint64_t h = hash64((uint64_t)key) & (A.ring.C - 1);
    int64_t kk = A.ring.keys[(size_t)p * A.ring.C + h];
    uint64_t *c = probe_resolve(A.ring.keys + (size_t)p * A.ring.C,
                                A.ring.state + (size_t)p * A.ring.C * 2,
                                A.ring.C, A.ring.err, key, h, kk);
    if (c) {
        atomicAdd((unsigned long long *)c, 1ULL);
        last_key = key;
        last_pane = p;
        last_cnt = c;
    }
}

/* phase A of one row: bin, late-drop, min fold, tag claim, sentinel-key
 * special case.  Returns false when the row needs no table update. */
__device__ inline bool row_prep(const UpdateArgs &A, uint64_t traw,
                                int64_t key, uint64_t &local_min,
                                uint64_t &last_bin, uint32_t &pane) {
    uint64_t t = traw + A.ts_offset;
    uint64_t q = div_slide(t, A.slide, A.slide_inv);
    uint64_t bin = q * A.slide;
    if (A.has_wm && bin < A.wm_bin) return false;
    if (bin < local_min) local_min = bin;
    pane = (uint32_t)(q & (A.ring.R - 1));
    if (bin != last_bin) {
        /* one leader lane claims for the wave: every thread's FIRST row
         * takes this path, and a per-thread volatile tag read serialized
         * the whole grid on one address (measured: launch time grew
         * linearly with block count) */
        claim_tag_wave(A.ring.tag, pane, bin, EMPTY_TAG, A.ring.err);
        last_bin = bin;
    }
    if (key == EMPTY_KEY) {
        atomicExch(&A.ring.spec_used[pane], 1u);
        atomicAdd((unsigned long long *)(A.ring.spec_state + (size_t)pane * 2),
                  1ULL);
        return false;
    }
    return true;
}

/* tiny per-block hot cache (direct-mapped LDS): absorbs the wave-uniform
 * nexmark hot key, whose same-address global atomics otherwise serialize
 * the whole chip (measured: 200-1000 us/launch, worse with more blocks).
 * 256 slots -> the flush is only 256 upserts per block (the 1024-slot
 * staging table's flush was the old LDS kernel's main global cost).
 * Returns true when the row was absorbed. */
#define BATCH_LSLOTS 256
__device__ inline bool lds_hot_try(int64_t *ls_key, uint32_t *ls_pane,
                                   unsigned long long *ls_cnt, int64_t key,
                                   uint32_t pane, uint32_t cnt) {
    uint32_t s = (uint32_t)hash64((uint64_t)key * 2654435761u + pane) &
                 (BATCH_LSLOTS - 1);
    int64_t lk = ls_key[s];
    if (lk == EMPTY_KEY) {
        int64_t old = (int64_t)atomicCAS((unsigned long long *)&ls_key[s],
                                         (unsigned long long)EMPTY_KEY,
                                         (unsigned long long)key);
        if (old == EMPTY_KEY) {
            ls_pane[s] = pane;
            atomicAdd(&ls_cnt[s], (unsigned long long)cnt);
            return true;
        }
        lk = old;
    }
    /* a stale PANE_UNSET read sends the row to the global path — safe */
    if (lk == key && ls_pane[s] == pane) {
        atomicAdd(&ls_cnt[s], (unsigned long long)cnt);
        return true;
    }
    return false;
}

/* Q rows per thread per iteration (8, 12 or 16).  87% of the wave time of
 * the narrow (Q = 2, 4) forms this replaced was parked on memory waits
 * (SQ_WAIT_ANY, profiles/r02e) — wider groups put more independent probe
 * loads in flight per thread.  The last n_rows % Q rows are left to a
 * separate scalar launch from the host: a device-side tail call forced
 * caller-save scratch spills into the hot loop. */
template <int Q>
__global__ void __launch_bounds__(256)
k_update_batch_n(UpdateArgs A) {
    __shared__ int64_t ls_key[BATCH_LSLOTS];
    __shared__ uint32_t ls_pane[BATCH_LSLOTS];
    __shared__ unsigned long long ls_cnt[BATCH_LSLOTS];
    for (int i = threadIdx.x; i < BATCH_LSLOTS; i += blockDim.x) {
        ls_key[i] = EMPTY_KEY;
        ls_pane[i] = PANE_UNSET;
        ls_cnt[i] = 0;
    }
    __syncthreads();
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    uint64_t local_min = ~0ULL, last_bin = EMPTY_TAG;
    int64_t last_key = EMPTY_KEY;
    uint32_t last_pane = PANE_UNSET;
    uint64_t *last_cnt = nullptr;
    int64_t nq = A.n_rows / Q;
    const uint64_t m = A.ring.C - 1;
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < nq;
         v += stride) {
        int64_t key[Q];
        uint64_t traw[Q];
#pragma unroll
        for (int j = 0; j < Q / 2; j++) {
            ulonglong2 tp = ((const ulonglong2 *)A.ts_col)[(Q / 2) * v + j];
            ulonglong2 kp = ((const ulonglong2 *)A.key_col)[(Q / 2) * v + j];
            traw[2 * j] = tp.x;
            traw[2 * j + 1] = tp.y;
            key[2 * j] = (int64_t)kp.x;
            key[2 * j + 1] = (int64_t)kp.y;
        }
        bool need[Q];
        uint32_t pane[Q];
        uint32_t cnt[Q];
#pragma unroll
        for (int j = 0; j < Q; j++) {
            pane[j] = 0;
            need[j] = row_prep(A, traw[j], key[j], local_min, last_bin,
                               pane[j]);
            cnt[j] = 1;
        }
#pragma unroll
        for (int j = Q - 1; j >= 1; j--)
            if (need[j] && need[j - 1] && key[j] == key[j - 1] &&
                pane[j] == pane[j - 1]) {
                cnt[j - 1] += cnt[j];
                need[j] = false;
            }
#pragma unroll
        for (int j = 0; j < Q; j++)
            if (need[j] && key[j] == last_key && pane[j] == last_pane &&
                last_cnt) {
                atomicAdd((unsigned long long *)last_cnt,
                          (unsigned long long)cnt[j]);
                need[j] = false;
            }
#pragma unroll
        for (int j = 0; j < Q; j++)
            if (need[j] &&
                lds_hot_try(ls_key, ls_pane, ls_cnt, key[j], pane[j],
                            cnt[j]))
                need[j] = false;
        uint64_t h[Q];
        int64_t firstk[Q];
#pragma unroll
        for (int j = 0; j < Q; j++)
            if (need[j]) {
                h[j] = hash64((uint64_t)key[j]) & m;
                firstk[j] = A.ring.keys[(size_t)pane[j] * A.ring.C + h[j]];
            }
#pragma unroll
        for (int j = 0; j < Q; j++) {
            if (!need[j]) continue;
            uint64_t *c = probe_resolve(
                A.ring.keys + (size_t)pane[j] * A.ring.C,
                A.ring.state + (size_t)pane[j] * A.ring.C * 2, A.ring.C,
                A.ring.err, key[j], h[j], firstk[j]);
            if (c) {
                atomicAdd((unsigned long long *)c,
                          (unsigned long long)cnt[j]);
                last_key = key[j];
                last_pane = pane[j];
                last_cnt = c;
            }
        }
    }
    fold_min_bin(local_min, A.ring.min_bin);
    __syncthreads();
    for (int s = threadIdx.x; s < BATCH_LSLOTS; s += blockDim.x) {
        int64_t key = ls_key[s];
        if (key == EMPTY_KEY) continue;
        uint32_t p = ls_pane[s];
        uint64_t h = hash64((uint64_t)key) & m;
        int64_t kk = A.ring.keys[(size_t)p * A.ring.C + h];
        uint64_t *c = probe_resolve(A.ring.keys + (size_t)p * A.ring.C,
                                    A.ring.state + (size_t)p * A.ring.C * 2,
                                    A.ring.C, A.ring.err, key, h, kk);
        if (c) atomicAdd((unsigned long long *)c, ls_cnt[s]);
    }
}

template __global__ void k_update_batch_n<8>(UpdateArgs);
template __global__ void k_update_batch_n<12>(UpdateArgs);
template __global__ void k_update_batch_n<16>(UpdateArgs);

/* ------------------------------------------------------------------ */
/* Tile update kernel (UPD_TILE, the default for the keyed single-COUNT
 * shape).  A time-ordered stream is local: all occurrences of a nexmark
 * cold key fall inside one ~1.5K-row stretch of the input, so a block that
 * owns a CONTIGUOUS span of rows sees every occurrence of most of its keys.
 * Block b owns row-vectors [b*S*256, (b+1)*S*256): S consecutive sub-tiles
 * of 256 x Q rows, aggregated into one hashed linear-probing LDS table
 * that lives for the whole span and is flushed once.  Rows that find no
 * slot within PROBES take k_update_batch_n's MLP-batched global path.
 * Counts model and measurements: profiles/tile_update_note.md. */

/* Claim protocol as in lds_update_row: CAS the key, then publish the pane.
 * A reader that sees the key with the pane still unset (or another pane)
 * moves on to the next probe; it never adds into a slot whose pane it
 * cannot see.  One (key, pane) may so end up in two slots — harmless, the
 * flush adds both.  Returns true when the rows were absorbed. */
template <int SLOTS, int PROBES>
__device__ inline bool lds_tile_try(int64_t *ls_key, uint32_t *ls_pane,
                                    uint32_t *ls_cnt, int64_t key,
                                    uint32_t pane, uint32_t cnt) {
    uint32_t h = (uint32_t)hash64((uint64_t)key * 2654435761u + pane);
#pragma unroll
    for (int pr = 0; pr < PROBES; pr++) {
        uint32_t s = (h + pr) & (SLOTS - 1);
        int64_t lk = ls_key[s];
        if (lk == EMPTY_KEY) {
            int64_t old = (int64_t)atomicCAS((unsigned long long *)&ls_key[s],
                                             (unsigned long long)EMPTY_KEY,
                                             (unsigned long long)key);
            if (old == EMPTY_KEY) {
                ls_pane[s] = pane;
                atomicAdd(&ls_cnt[s], cnt);
                return true;
            }
            lk = old;
        }
        if (lk == key && ls_pane[s] == pane) {
            atomicAdd(&ls_cnt[s], cnt);
            return true;
        }
    }
    return false;
}

template <int Q, int SLOTS, int PROBES>
__global__ void __launch_bounds__(256)
k_update_tile(UpdateArgs A, int S) {
    __shared__ int64_t ls_key[SLOTS];
    __shared__ uint32_t ls_pane[SLOTS];
    __shared__ uint32_t ls_cnt[SLOTS];
    for (int i = threadIdx.x; i < SLOTS; i += 256) {
        ls_key[i] = EMPTY_KEY;
        ls_pane[i] = PANE_UNSET;
        ls_cnt[i] = 0;
    }
    __syncthreads();
    uint64_t local_min = ~0ULL, last_bin = EMPTY_TAG;
    int64_t last_key = EMPTY_KEY;
    uint32_t last_pane = PANE_UNSET;
    uint64_t *last_cnt = nullptr;
    const int64_t nq = A.n_rows / Q;
    const uint64_t m = A.ring.C - 1;
    int64_t v = (int64_t)blockIdx.x * S * 256 + threadIdx.x;
    for (int t = 0; t < S && v < nq; t++, v += 256) {
        int64_t key[Q];
        uint64_t traw[Q];
#pragma unroll
        for (int j = 0; j < Q / 2; j++) {
            ulonglong2 tp = ((const ulonglong2 *)A.ts_col)[(Q / 2) * v + j];
            ulonglong2 kp = ((const ulonglong2 *)A.key_col)[(Q / 2) * v + j];
            traw[2 * j] = tp.x;
            traw[2 * j + 1] = tp.y;
            key[2 * j] = (int64_t)kp.x;
            key[2 * j + 1] = (int64_t)kp.y;
        }
        bool need[Q];
        uint32_t pane[Q];
        uint32_t cnt[Q];
#pragma unroll
        for (int j = 0; j < Q; j++) {
            pane[j] = 0;
            need[j] = row_prep(A, traw[j], key[j], local_min, last_bin,
                               pane[j]);
            cnt[j] = 1;
        }
#pragma unroll
        for (int j = Q - 1; j >= 1; j--)
            if (need[j] && need[j - 1] && key[j] == key[j - 1] &&
                pane[j] == pane[j - 1]) {
                cnt[j - 1] += cnt[j];
                need[j] = false;
            }
#pragma unroll
        for (int j = 0; j < Q; j++)
            if (need[j] && key[j] == last_key && pane[j] == last_pane &&
                last_cnt) {
                atomicAdd((unsigned long long *)last_cnt,
                          (unsigned long long)cnt[j]);
                need[j] = false;
            }
#pragma unroll
        for (int j = 0; j < Q; j++)
            if (need[j] &&
                lds_tile_try<SLOTS, PROBES>(ls_key, ls_pane, ls_cnt, key[j],
                                            pane[j], cnt[j]))
                need[j] = false;
        uint64_t h[Q];
        int64_t firstk[Q];
#pragma unroll
        for (int j = 0; j < Q; j++)
            if (need[j]) {
                h[j] = hash64((uint64_t)key[j]) & m;
                firstk[j] = A.ring.keys[(size_t)pane[j] * A.ring.C + h[j]];
            }
#pragma unroll
        for (int j = 0; j < Q; j++) {
            if (!need[j]) continue;
            uint64_t *c = probe_resolve(
                A.ring.keys + (size_t)pane[j] * A.ring.C,
                A.ring.state + (size_t)pane[j] * A.ring.C * 2, A.ring.C,
                A.ring.err, key[j], h[j], firstk[j]);
            if (c) {
                atomicAdd((unsigned long long *)c,
                          (unsigned long long)cnt[j]);
                last_key = key[j];
                last_pane = pane[j];
                last_cnt = c;
            }
        }
    }
    fold_min_bin(local_min, A.ring.min_bin);
    __syncthreads();
    /* flush: each thread owns SLOTS/256 slots and issues the first-probe
     * key loads of all its occupied slots before resolving any of them
     * (the row loop's trick; the old flush was one dependent probe chain
     * per slot) */
    constexpr int NF = SLOTS / 256;
    int64_t fkey[NF], ffirst[NF];
    uint32_t fpane[NF];
    uint64_t fh[NF];
#pragma unroll
    for (int j = 0; j < NF; j++) {
        int s = threadIdx.x + j * 256;
        fkey[j] = ls_key[s];
        fpane[j] = ls_pane[s];
        fh[j] = 0;
        ffirst[j] = 0;
        if (fkey[j] != EMPTY_KEY) {
            fh[j] = hash64((uint64_t)fkey[j]) & m;
            ffirst[j] = A.ring.keys[(size_t)fpane[j] * A.ring.C + fh[j]];
        }
    }
#pragma unroll
    for (int j = 0; j < NF; j++) {
        if (fkey[j] == EMPTY_KEY) continue;
        uint64_t *c = probe_resolve(
            A.ring.keys + (size_t)fpane[j] * A.ring.C,
            A.ring.state + (size_t)fpane[j] * A.ring.C * 2, A.ring.C,
            A.ring.err, fkey[j], fh[j], ffirst[j]);
        if (c)
            atomicAdd((unsigned long long *)c,
                      (unsigned long long)ls_cnt[threadIdx.x + j * 256]);
    }
}

/* 1024 slots x 4 probes won the {512,1024,2048} x {2,4} sweep at the bench
 * shape (16 KB of LDS per block) */
#define TILE_SLOTS 1024
#define TILE_PROBES 4
template __global__ void k_update_tile<8, TILE_SLOTS, TILE_PROBES>(UpdateArgs,
                                                                   int);
template __global__ void k_update_tile<12, TILE_SLOTS, TILE_PROBES>(UpdateArgs,
                                                                    int);
template __global__ void k_update_tile<16, TILE_SLOTS, TILE_PROBES>(UpdateArgs,
                                                                    int);

/* scalar kernel of the batch and tile kinds (tail rows, misaligned columns) */
__global__ void __launch_bounds__(256)
k_update_batch_scalar(UpdateArgs A) {
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    uint64_t local_min = ~0ULL, last_bin = EMPTY_TAG;
    int64_t last_key = EMPTY_KEY;
    uint32_t last_pane = PANE_UNSET;
    uint64_t *last_cnt = nullptr;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         i < A.n_rows; i += stride)
        batch_row_scalar(A, (uint64_t)A.ts_col[i], A.key_col[i], local_min,
                         last_bin, last_key, last_pane, last_cnt);
    fold_min_bin(local_min, A.ring.min_bin);
}

/* The pane's tag must become EMPTY only after EVERY block's plane clears
 * are agent-visible: with the fire stream overlapping updates, a
 * concurrent update kernel may claim the slot the instant the tag reads
 * empty, and a tag cleared early would hand it a half-cleared table
 * (silent corruption).  The plane-clear kernels therefore do NOT touch
 * the tag; k_retire_tag follows them on the same stream, and the kernel
 * boundary is the grid-wide completion + release point.  (A grid-wide
 * done counter was measured instead: 1024 same-address returning atomics
 * serialize at ~0.3 us each -- it turned a ~5 us retire into a fire-
 * stream-dominating one and cost 25% whole-job.) */
struct RetireTagsArgs {
    uint64_t *tag;            /* [R] */
    uint32_t *spec_used;      /* [R] */
    uint64_t *spec_state;     /* [R][na2] */
    int na2;
    int n;
    uint32_t slot[8];
};

__global__ void k_retire_tags(RetireTagsArgs A) {
    for (int i = 0; i < A.n; i++) {
        uint32_t p = A.slot[i];
        A.spec_used[p] = 0;
        for (int w = 0; w < A.na2; w++)
            A.spec_state[(size_t)p * A.na2 + w] = 0;
        __hip_atomic_store((unsigned long long *)(A.tag + p),
                           (unsigned long long)EMPTY_TAG, __ATOMIC_RELEASE,
                           __HIP_MEMORY_SCOPE_AGENT);
    }
}

/* one-launch pane retire (plane clears): keys to 0xFF,
 * states to 0, scalar metadata — replaces two fill launches plus a
 * metadata kernel (~5 us each on a busy stream) per retire */
__global__ void __launch_bounds__(256)
k_retire_all(int64_t *keys, uint64_t *state, int64_t C, int na2) {
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    int64_t kv2 = C >> 1;          /* C is a power of two >= 2 */
    ulonglong2 ff, zz;
    ff.x = ff.y = ~0ULL;
    zz.x = zz.y = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         i < kv2; i += stride)
        ((ulonglong2 *)keys)[i] = ff;
    int64_t sv2 = (C * na2) >> 1;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         i < sv2; i += stride)
        ((ulonglong2 *)state)[i] = zz;
}

/* ------------------------------------------------------------------ */
/* Multi-column keys (n_keys 2..4): a device key dictionary normalizes
 * each composite key to a 64-bit id (its dictionary slot), and the
 * single-key engine runs unchanged on the ids; emissions decode ids back
 * to the original tuples.  This mirrors the reference's own key
 * normalization — it converts every key tuple to Arrow Row bytes before
 * the state map (expiring_time_key_map.rs:1008-1049) — with the
 * normalization done once, on device.  Exactness: slots are claimed by
 * digest CAS but verified by full-tuple compare; a digest collision just
 * probes on.  The dictionary never evicts (ids must stay stable for live
 * panes); capacity is 4x the pane table and exhaustion is a loud error. */
#define ERR_DICT_FULL 7
#define ERR_DICT_SPIN 8

struct DictEncArgs {
    const int64_t *kcols[4];
    int32_t nk;
    int64_t n_rows;
    int64_t *digest;     /* [D]; EMPTY_KEY = free (stored digests have the
                            top bit cleared, so they never equal -1) */
    int64_t *dkeys;      /* [D][nk] */
    uint32_t *ready;     /* [D] tuple words published */
    int64_t *ids;        /* [n_rows] out */
    uint32_t D;
    int *err;
};

__device__ inline uint64_t dev_hash_tuple(const int64_t *key, int nk) {
    uint64_t h = hash64((uint64_t)key[0]);
    for (int k = 1; k < nk; k++) h = hash64(h ^ (uint64_t)key[k]);
    return h;
}

__global__ void __launch_bounds__(256)
k_dict_encode(DictEncArgs A) {
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const uint64_t m = A.D - 1;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         r < A.n_rows; r += stride) {
        int64_t key[4];
        for (int k = 0; k < A.nk; k++) key[k] = A.kcols[k][r];
        uint64_t h = dev_hash_tuple(key, A.nk);
        int64_t dg = (int64_t)(h & 0x7FFFFFFFFFFFFFFFULL);
        bool done = false;
        /* outer retry loop instead of a divergent spin-wait: a lane that
         * finds a claimed-but-unpublished slot backs off so the wave
         * reconverges and the writer lane's stores can execute */
        for (int tries = 0; tries < (1 << 20) && !done; tries++) {
            uint64_t i = h & m;
            for (uint32_t probes = 0; probes < A.D; probes++) {
                int64_t cur = A.digest[i];
                if (cur == EMPTY_KEY) {
                    int64_t old = (int64_t)atomicCAS(
                        (unsigned long long *)&A.digest[i],
                        (unsigned long long)EMPTY_KEY,
                        (unsigned long long)dg);
                    if (old == EMPTY_KEY) {
                        for (int k = 0; k < A.nk; k++)
                            A.dkeys[i * A.nk + k] = key[k];
                        /* agent-scope release: the tuple words must be
                         * visible before the flag (a relaxed flag let
                         * readers see stale L1 tuple lines, falsely
                         * mismatch, and claim a SECOND id for the same
                         * key — observed as split aggregates) */
                        __hip_atomic_store(&A.ready[i], 1u,
                                           __ATOMIC_RELEASE,
                                           __HIP_MEMORY_SCOPE_AGENT);
                        A.ids[r] = (int64_t)i;
                        done = true;
                        break;
                    }
                    cur = old;
                }
                if (cur == dg) {
                    if (!__hip_atomic_load(&A.ready[i], __ATOMIC_ACQUIRE,
                                           __HIP_MEMORY_SCOPE_AGENT))
                        break;   /* writer not published yet: retry row */
                    bool eq = true;
                    for (int k = 0; k < A.nk && eq; k++)
                        eq = A.dkeys[i * A.nk + k] == key[k];
                    if (eq) {
                        A.ids[r] = (int64_t)i;
                        done = true;
                        break;
                    }
                    /* digest collision of a different tuple: probe on */
                }
                i = (i + 1) & m;
                if (probes + 1 == A.D) {
                    *A.err = ERR_DICT_FULL;
                    A.ids[r] = 0;
                    done = true;
                    break;
                }
            }
        }
        if (!done) {
            *A.err = ERR_DICT_SPIN;
            A.ids[r] = 0;
        }
    }
}

/* expand an id column back to the original key tuple columns */
struct DictDecArgs {
    const int64_t *ids;
    const unsigned long long *n;   /* device row count */
    const int64_t *dkeys;
    int32_t nk;
    int64_t *out[4];
};

__global__ void __launch_bounds__(256)
k_dict_decode(DictDecArgs A) {
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    int64_t n = (int64_t)*A.n;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n;
         r += stride) {
        int64_t id = A.ids[r];
        for (int k = 0; k < A.nk; k++)
            A.out[k][r] = A.dkeys[id * A.nk + k];
    }
}

/* ------------------------------------------------------------------ */
/* K4: merge source panes into the merge table.                        */

struct MergeArgs {
    DeviceRing ring;
    AggSpec agg;
    int64_t  *m_keys;     /* [CM] */
    uint64_t *m_state;    /* [CM][n_aggs][2] */
    uint32_t *m_spec_used;
    uint64_t *m_spec_state;
    uint32_t  CM;
    int32_t   n_src;
    uint32_t  src[64];    /* ring slots to merge */
};

__global__ void __launch_bounds__(256)
k_merge(MergeArgs M) {
    size_t total = (size_t)M.n_src * M.ring.C;
    size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
         i < total; i += stride) {
        uint32_t p = M.src[i / M.ring.C];
        size_t slot = i % M.ring.C;
        int64_t key = M.ring.keys[(size_t)p * M.ring.C + slot];
        if (key == EMPTY_KEY) continue;
        int64_t d = table_upsert(M.m_keys, M.CM, key, M.ring.err);
        if (d < 0) continue;
        atomic_merge(M.m_state + (size_t)d * M.agg.n_aggs * 2,
                     M.ring.state +
                         ((size_t)p * M.ring.C + slot) * M.agg.n_aggs * 2,
                     M.agg);
    }
    /* special (key == EMPTY_KEY sentinel value) entries */
    if (blockIdx.x == 0 && threadIdx.x < (unsigned)M.n_src) {
        uint32_t p = M.src[threadIdx.x];
        if (M.ring.spec_used[p]) {
            atomicExch(M.m_spec_used, 1u);
            atomic_merge(M.m_spec_state,
                         M.ring.spec_state + (size_t)p * M.agg.n_aggs * 2,
                         M.agg);
        }
    }
}

/* ------------------------------------------------------------------ */
/* K5: compact occupied merge-table slots into output columns.
 * Output column order: [key?], aggs..., window_start, window_end, _ts.  */

struct CompactArgs {
    const int64_t  *m_keys;
    const uint64_t *m_state;
    const uint32_t *m_spec_used;
    const uint64_t *m_spec_state;
    uint32_t  CM;
    AggSpec   agg;
    int32_t   n_keys;
    int32_t   raw_states;  /* 1: emit encoded->raw partial states
                              (checkpoint drain layout) instead of finals */
    uint64_t  win_start, win_end;
    int64_t  *out[16];     /* device output columns */
    unsigned long long *n_out;
};

__device__ inline void emit_row(const CompactArgs &C, int64_t key,
                                const uint64_t *st, int64_t r) {
    int col = 0;
    if (C.n_keys) C.out[col++][r] = key;
    for (int a = 0; a < C.agg.n_aggs; a++) {
        uint64_t w0 = st[2 * a];
        switch (C.agg.op[a]) {
        case AMD_AGG_COUNT:
        case AMD_AGG_SUM:
            C.out[col++][r] = (int64_t)w0;   /* SUM f64: raw double bits */
            break;
        case AMD_AGG_MIN:
        case AMD_AGG_MAX:
            C.out[col++][r] = dec_word(C.agg.op[a], C.agg.isf[a], w0);
            break;
        case AMD_AGG_AVG:
            if (C.raw_states) {
                C.out[col++][r] = (int64_t)w0;
                C.out[col++][r] = (int64_t)st[2 * a + 1];  /* f64 bits */
            } else {
                double v = w0 ? (*(const double *)(st + 2 * a + 1)) /
                                    (double)(int64_t)w0
                              : 0.0;
                int64_t b;
                memcpy(&b, &v, 8);
                C.out[col++][r] = b;
            }
            break;
        }
    }
    if (!C.raw_states) {
        C.out[col++][r] = (int64_t)C.win_start;
        C.out[col++][r] = (int64_t)C.win_end;
        C.out[col++][r] = (int64_t)(C.win_end - 1);
    } else {
        C.out[col++][r] = (int64_t)C.win_start;  /* bin timestamp */
    }
}

__global__ void __launch_bounds__(256)
k_compact(CompactArgs C) {
    /* Two passes with ONE global cursor atomic per block: same-address
     * global atomics cost ~12 ns each across the chip, so per-row (651K) or
     * even per-wave (16K) cursors dominated this kernel (~200 us).  Pass 1
     * counts the block's live slots, one atomicAdd claims the block's output
     * range, pass 2 emits at LDS-cursor positions (LDS atomics are cheap). */
    __shared__ unsigned long long blk_base;
    __shared__ unsigned int blk_cnt;
    size_t stride = (size_t)gridDim.x * blockDim.x;
    if (threadIdx.x == 0) blk_cnt = 0;
    __syncthreads();
    unsigned int mine = 0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < C.CM;
         i += stride)
        mine += (C.m_keys[i] != EMPTY_KEY);
    for (int off = 32; off; off >>= 1)
        mine += (unsigned)__shfl_down((int)mine, off, 64);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(&blk_cnt, mine);
    __syncthreads();
    if (threadIdx.x == 0) {
        blk_base = blk_cnt ? atomicAdd(C.n_out,
                                       (unsigned long long)blk_cnt)
                           : 0;
        blk_cnt = 0;
    }
    __syncthreads();
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < C.CM;
         i += stride) {
        int64_t key = C.m_keys[i];
        if (key == EMPTY_KEY) continue;
        int64_t r = (int64_t)(blk_base + atomicAdd(&blk_cnt, 1u));
        emit_row(C, key, C.m_state + i * C.agg.n_aggs * 2, r);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && *C.m_spec_used)
        emit_row(C, EMPTY_KEY, C.m_spec_state,
                 (int64_t)atomicAdd(C.n_out, 1ULL));
}

__global__ void k_accum(unsigned long long *acc,
                        const unsigned long long *n) {
    *acc += *n;
}

/* ------------------------------------------------------------------ */
/* K4+K5 fused, hash-aligned: each workgroup owns a disjoint range of HOME
 * slots (hash(key) & mask in [a, a+RANGE)).  It scans that range (+ the
 * MAX_PROBES displacement overscan) of every source pane, dedupes and sums
 * the owned keys in an LDS table, and emits final rows directly -- no
 * global merge table, no state atomics, ONE output-cursor atomic per
 * workgroup.  Used when n_aggs <= MF_MAX_AGGS (LDS budget) and not
 * draining raw states; the legacy merge+compact path covers the rest. */
#define MF_RANGE 256u
#define MF_SLOTS 2048
#define MF_MAX_AGGS 2
#define ERR_MF_OVERFLOW 6

struct MergeFusedArgs {
    DeviceRing ring;
    AggSpec agg;
    int32_t n_src;
    uint32_t src[64];
    uint64_t win_start, win_end;
    int32_t n_keys;
    uint32_t range;     /* home slots per WG; gridDim.x == C / range */
    int64_t *out[16];
    unsigned long long *n_out;
    unsigned long long *accum;  /* running emitted-rows accumulator (may be
                                   null); folded in here so the separate
                                   k_accum launch (~5 us) is not needed */
    /* closed-pane index (CPI): each closed pane compacted ONCE into
     * home-range-grouped dense {key, state} entries, so the five fires
     * that read it scan only occupied entries instead of the whole
     * sparse table + displacement overscan (the fire path was 52% of
     * GPU time on the sparse scan).  use_cpi covers n_src <= 16. */
    int32_t use_cpi;
    int32_t cpi_ew;   /* entry words: 1+1 when only word0 of a single agg
                         is live (COUNT/SUM/MIN/MAX), else 1+2*na */
    uint32_t cpi_range;  /* index granularity: the build runs one WG per
                            cpi_range home slots (smaller than the merge
                            range so the build grid can hide latency);
                            a merge WG reads range/cpi_range segments */
    const uint64_t *cpi_entries[16];   /* [nr][cpi_range][cpi_ew] */
    const uint32_t *cpi_cnt[16];       /* [nr] entries per sub-range */
};

/* Closed-pane index build: one workgroup per home range.  Linear probing
 * bounds a key's stored slot to [home, home + MAX_PROBES], so range r's
 * keys all sit in slots [r*range, (r+1)*range + MAX_PROBES): one
 * overscan sweep per PANE (instead of one per fire) collects them into a
 * dense per-range segment.  Per-range capacity equals `range` (pane load
 * factor is bounded well below 1 by construction; exceeding it is a
 * loud error). */
#define CPI_MAX_NR 8192

struct CpiBuildArgs {
    const int64_t *keys;      /* pane planes in the ring */
    const uint64_t *state;
    uint32_t C;
    int32_t ew;               /* entry words (see MergeFusedArgs.cpi_ew) */
    int32_t na;
    uint32_t range;
    uint32_t nr;              /* C / range */
    uint32_t *cnt;            /* [nr] entries per range (output) */
    uint64_t *entries;        /* [nr][range][1 + 2*na] */
    int *err;
};

__global__ void __launch_bounds__(256)
k_cpi_build(CpiBuildArgs A) {
    __shared__ uint32_t lcur;
    if (threadIdx.x == 0) lcur = 0;
    __syncthreads();
    const uint32_t mask = A.C - 1;
    const uint32_t a = blockIdx.x * A.range;
    const uint32_t span = A.range + MAX_PROBES;
    const int ew = A.ew;
    uint64_t *dst = A.entries + (size_t)blockIdx.x * A.range * ew;
    auto emit = [&](int64_t key, uint32_t idx) {
        if (key == EMPTY_KEY) return;
        uint32_t rel = ((uint32_t)hash64((uint64_t)key) - a) & mask;
        if (rel >= A.range) return;
        uint32_t pos = atomicAdd(&lcur, 1u);
        if (pos >= A.range) { *A.err = ERR_MF_OVERFLOW; return; }
        uint64_t *e = dst + (size_t)pos * ew;
        if (ew == 2) {
            ulonglong2 v;
            v.x = (uint64_t)key;
            v.y = A.state[(size_t)idx * A.na * 2];
            *(ulonglong2 *)e = v;
        } else {
            e[0] = (uint64_t)key;
            for (int w = 0; w < 2 * A.na; w++)
                e[1 + w] = A.state[(size_t)idx * A.na * 2 + w];
        }
    };
    /* 2 keys per 16 B load (a and span are even and an even idx never
     * straddles the wrap, same argument as the merge's pair scan); four
     * pair loads issued together so the scan is not one long dependent
     * miss chain */
    const uint32_t step = 2 * blockDim.x;
    uint32_t t = 2 * threadIdx.x;
    for (; t + 3 * step < span; t += 4 * step) {
        uint32_t i0 = (a + t) & mask;
        uint32_t i1 = (a + t + step) & mask;
        uint32_t i2 = (a + t + 2 * step) & mask;
        uint32_t i3 = (a + t + 3 * step) & mask;
        ulonglong2 k0 = *(const ulonglong2 *)&A.keys[i0];
        ulonglong2 k1 = *(const ulonglong2 *)&A.keys[i1];
        ulonglong2 k2 = *(const ulonglong2 *)&A.keys[i2];
        ulonglong2 k3 = *(const ulonglong2 *)&A.keys[i3];
        emit((int64_t)k0.x, i0); emit((int64_t)k0.y, i0 + 1);
        emit((int64_t)k1.x, i1); emit((int64_t)k1.y, i1 + 1);
        emit((int64_t)k2.x, i2); emit((int64_t)k2.y, i2 + 1);
        emit((int64_t)k3.x, i3); emit((int64_t)k3.y, i3 + 1);
    }
    for (; t < span; t += step) {
        uint32_t idx = (a + t) & mask;
        ulonglong2 kv = *(const ulonglong2 *)&A.keys[idx];
        emit((int64_t)kv.x, idx);
        emit((int64_t)kv.y, idx + 1);
    }
    __syncthreads();
    if (threadIdx.x == 0) A.cnt[blockIdx.x] = lcur < A.range ? lcur : A.range;
}

template <int SLOTS>
__global__ void __launch_bounds__(256)
k_merge_fused(MergeFusedArgs M) {
    __shared__ int64_t lkey[SLOTS];
    extern __shared__ uint64_t lst[];    /* [SLOTS][n_aggs][2], or
                                            [SLOTS] single words when the
                                            lone aggregate uses only word0
                                            (compact: halves the LDS and
                                            lifts the WGs/CU cap) */
    __shared__ unsigned long long blk_base;
    __shared__ unsigned int blk_cnt;
    const int na = M.agg.n_aggs;
    const int compact = (M.use_cpi && M.cpi_ew == 2);
    const int sw = compact ? 1 : na * 2;
    const uint32_t C = M.ring.C, mask = C - 1;
    for (int i = threadIdx.x; i < SLOTS; i += blockDim.x) {
        lkey[i] = EMPTY_KEY;
        for (int w = 0; w < sw; w++) lst[(size_t)i * sw + w] = 0;
    }
    if (threadIdx.x == 0) blk_cnt = 0;
    __syncthreads();
    uint32_t a = blockIdx.x * M.range;           /* gridDim.x == C/range */
    uint32_t span = M.range + MAX_PROBES;        /* displacement overscan */
    for (int p = 0; p < M.n_src; p++) {
        const int64_t *keys = M.ring.keys + (size_t)M.src[p] * C;
        const uint64_t *st = M.ring.state + (size_t)M.src[p] * C * na * 2;
        auto fold = [&](int64_t key, const uint64_t *stv, bool own) {
            if (key == EMPTY_KEY) return;
            if (!own) {
                uint32_t rel = ((uint32_t)hash64((uint64_t)key) - a) & mask;
                if (rel >= M.range) return;      /* another WG owns it */
            }
            /* LDS upsert */
            uint32_t h = (uint32_t)hash64((uint64_t)key * 0x9e3779b1u) &
                         (SLOTS - 1);
            int64_t slot = -1;
            for (int pr = 0; pr < SLOTS && slot < 0; pr++) {
                uint32_t sidx = (h + pr) & (SLOTS - 1);
                int64_t k = lkey[sidx];
                if (k == key) {
                    slot = sidx;
                } else if (k == EMPTY_KEY) {
                    int64_t old = (int64_t)atomicCAS(
                        (unsigned long long *)&lkey[sidx],
                        (unsigned long long)EMPTY_KEY,
                        (unsigned long long)key);
                    if (old == EMPTY_KEY || old == key) slot = sidx;
                }
            }
            if (slot < 0) { *M.ring.err = ERR_MF_OVERFLOW; return; }
            uint64_t *d = lst + (size_t)slot * sw;
            if (compact) {   /* single live word: fold without the pair
                                stride atomic_merge assumes */
                switch (M.agg.op[0]) {
                case AMD_AGG_SUM:
                    if (M.agg.isf[0]) {
                        atomicAdd((double *)d, *(const double *)stv);
                        return;
                    }
                    /* fallthrough: integer add */
                case AMD_AGG_COUNT:
                    atomicAdd((unsigned long long *)d,
                              (unsigned long long)stv[0]);
                    return;
                default:   /* MIN/MAX: order-preserving u64 encodings */
                    atomicMax((unsigned long long *)d,
                              (unsigned long long)stv[0]);
                    return;
                }
            }
            atomic_merge(d, stv, M.agg);
        };
        if (M.use_cpi) {
            /* dense home-range-grouped entries: only occupied slots read,
             * ownership established at build time */
            const int ew = M.cpi_ew;
            const uint32_t nsub = M.range / M.cpi_range;
            for (uint32_t j = 0; j < nsub; j++) {
                uint32_t seg = blockIdx.x * nsub + j;
                const uint32_t n_e = M.cpi_cnt[p][seg];
                const uint64_t *ent = M.cpi_entries[p] +
                                      (size_t)seg * M.cpi_range * ew;
                if (ew == 2) {
                    /* 16 B entries; 4 loads issued together per thread
                     * (memory-level parallelism -- the single-load loop
                     * serializes a ~900-cycle miss against LDS work,
                     * exactly the update kernel's Q-batching lesson) */
                    const uint32_t stride = blockDim.x;
                    uint32_t t = threadIdx.x;
                    for (; t + 3 * stride < n_e; t += 4 * stride) {
                        ulonglong2 e0 = ((const ulonglong2 *)ent)[t];
                        ulonglong2 e1 =
                            ((const ulonglong2 *)ent)[t + stride];
                        ulonglong2 e2 =
                            ((const ulonglong2 *)ent)[t + 2 * stride];
                        ulonglong2 e3 =
                            ((const ulonglong2 *)ent)[t + 3 * stride];
                        uint64_t w;
                        w = e0.y; fold((int64_t)e0.x, &w, true);
                        w = e1.y; fold((int64_t)e1.x, &w, true);
                        w = e2.y; fold((int64_t)e2.x, &w, true);
                        w = e3.y; fold((int64_t)e3.x, &w, true);
                    }
                    for (; t < n_e; t += stride) {
                        ulonglong2 e = ((const ulonglong2 *)ent)[t];
                        uint64_t w0 = (uint64_t)e.y;
                        fold((int64_t)e.x, &w0, true);
                    }
                } else {
                    for (uint32_t t = threadIdx.x; t < n_e;
                         t += blockDim.x) {
                        const uint64_t *e = ent + (size_t)t * ew;
                        fold((int64_t)e[0], e + 1, true);
                    }
                }
            }
        } else {
            /* 2 keys per 16 B load: a and span are multiples of 2, and an
             * even idx never straddles the wrap, so the pair load is safe */
            for (uint32_t t = 2 * threadIdx.x; t < span;
                 t += 2 * blockDim.x) {
                uint32_t idx = (a + t) & mask;
                ulonglong2 kv = *(const ulonglong2 *)&keys[idx];
                fold((int64_t)kv.x, st + (size_t)idx * na * 2, false);
                fold((int64_t)kv.y, st + ((size_t)idx + 1) * na * 2, false);
            }
        }
    }
    __syncthreads();
    /* pass 1: count occupied LDS slots; one global cursor add per WG */
    unsigned int mine = 0;
    for (int i = threadIdx.x; i < SLOTS; i += blockDim.x)
        mine += (lkey[i] != EMPTY_KEY);
    for (int off = 32; off; off >>= 1)
        mine += (unsigned)__shfl_down((int)mine, off, 64);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(&blk_cnt, mine);
    __syncthreads();
    if (threadIdx.x == 0) {
        blk_base = blk_cnt ? atomicAdd(M.n_out,
                                       (unsigned long long)blk_cnt)
                           : 0;
        if (M.accum && blk_cnt)
            atomicAdd(M.accum, (unsigned long long)blk_cnt);
        blk_cnt = 0;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < SLOTS; i += blockDim.x) {
        int64_t key = lkey[i];
        if (key == EMPTY_KEY) continue;
        int64_t r = (int64_t)(blk_base + atomicAdd(&blk_cnt, 1u));
        const uint64_t *d = lst + (size_t)i * sw;
        int col = 0;
        if (M.n_keys) M.out[col++][r] = key;
        for (int ag = 0; ag < na; ag++) {
            uint64_t w0 = d[compact ? 0 : 2 * ag];
            switch (M.agg.op[ag]) {
            case AMD_AGG_COUNT:
            case AMD_AGG_SUM: M.out[col++][r] = (int64_t)w0; break;
            case AMD_AGG_MIN:
            case AMD_AGG_MAX:
                M.out[col++][r] = dec_word(M.agg.op[ag], M.agg.isf[ag], w0);
                break;
            case AMD_AGG_AVG: {
                double v = w0 ? (*(const double *)(d + 2 * ag + 1)) /
                                    (double)(int64_t)w0
                              : 0.0;
                int64_t b;
                memcpy(&b, &v, 8);
                M.out[col++][r] = b;
                break;
            }
            }
        }
        M.out[col++][r] = (int64_t)M.win_start;
        M.out[col++][r] = (int64_t)M.win_end;
        M.out[col][r] = (int64_t)(M.win_end - 1);
    }
    /* special (key == sentinel) entries: one extra row */
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        uint64_t spec[2 * AMD_MAX_AGGS] = {};
        int any = 0;
        for (int p = 0; p < M.n_src; p++) {
            uint32_t pp = M.src[p];
            if (!M.ring.spec_used[pp]) continue;
            any = 1;
            const uint64_t *st =
                M.ring.spec_state + (size_t)pp * na * 2;
            for (int ag = 0; ag < na; ag++) {
                switch (M.agg.op[ag]) {
                case AMD_AGG_COUNT:
                    spec[2 * ag] += st[2 * ag];
                    break;
                case AMD_AGG_SUM:
                    if (M.agg.isf[ag]) {
                        double x, y;
                        memcpy(&x, &spec[2 * ag], 8);
                        memcpy(&y, &st[2 * ag], 8);
                        x += y;
                        memcpy(&spec[2 * ag], &x, 8);
                    } else {
                        spec[2 * ag] += st[2 * ag];
                    }
                    break;
                case AMD_AGG_MIN:
                case AMD_AGG_MAX:
                    if (st[2 * ag] > spec[2 * ag]) spec[2 * ag] = st[2 * ag];
                    break;
                case AMD_AGG_AVG: {
                    spec[2 * ag] += st[2 * ag];
                    double x, y;
                    memcpy(&x, &spec[2 * ag + 1], 8);
                    memcpy(&y, &st[2 * ag + 1], 8);
                    x += y;
                    memcpy(&spec[2 * ag + 1], &x, 8);
                    break;
                }
                }
            }
        }
        if (any) {
            int64_t r = (int64_t)atomicAdd(M.n_out, 1ULL);
            if (M.accum) atomicAdd(M.accum, 1ULL);
            int col = 0;
            if (M.n_keys) M.out[col++][r] = EMPTY_KEY;
            for (int ag = 0; ag < na; ag++) {
                uint64_t w0 = spec[2 * ag];
                switch (M.agg.op[ag]) {
                case AMD_AGG_COUNT:
                case AMD_AGG_SUM: M.out[col++][r] = (int64_t)w0; break;
                case AMD_AGG_MIN:
                case AMD_AGG_MAX:
                    M.out[col++][r] = dec_word(M.agg.op[ag], M.agg.isf[ag],
                                               w0);
                    break;
                case AMD_AGG_AVG: {
                    double v = w0 ? (*(const double *)(spec + 2 * ag + 1)) /
                                        (double)(int64_t)w0
                                  : 0.0;
                    int64_t b;
                    memcpy(&b, &v, 8);
                    M.out[col++][r] = b;
                    break;
                }
                }
            }
            M.out[col++][r] = (int64_t)M.win_start;
            M.out[col++][r] = (int64_t)M.win_end;
            M.out[col][r] = (int64_t)(M.win_end - 1);
        }
    }
}

template __global__ void k_merge_fused<1024>(MergeFusedArgs);
template __global__ void k_merge_fused<2048>(MergeFusedArgs);
template __global__ void k_merge_fused<4096>(MergeFusedArgs);

/* Dual-window fused merge (COUNT-shaped panes only): two CONSECUTIVE
 * sliding windows fired in the same watermark group share all but one
 * source pane, so one kernel scans the union (6 pane segments instead of
 * 10) and maintains both windows' counts per key in LDS.  A key emits a
 * row per window where it has a nonzero count (COUNT >= 1 iff the key
 * occurs in any of that window's panes, so presence needs no extra
 * bits).  Emissions match two k_merge_fused launches up to row order
 * within the call (the batched-watermark API returns the group's fires
 * concatenated; order within the batch is not part of the contract). */
struct MergeDualArgs {
    DeviceRing ring;
    int32_t n_src;
    uint32_t src[16];
    uint64_t maskA, maskB;    /* src-index bitmasks of each window */
    uint64_t wsA, weA, wsB, weB;
    int32_t n_keys;
    uint32_t range;
    uint32_t cpi_range;
    int64_t *out[8];
    unsigned long long *n_out;
    unsigned long long *accum;
    const uint64_t *cpi_entries[16];
    const uint32_t *cpi_cnt[16];
};

template <int SLOTS>
__global__ void __launch_bounds__(256)
k_merge_dual(MergeDualArgs M) {
    __shared__ int64_t lkey[SLOTS];
    extern __shared__ uint64_t lst[];        /* [2][SLOTS] counts */
    __shared__ unsigned long long blk_base;
    __shared__ unsigned int blk_cnt;
    uint64_t *cA = lst, *cB = lst + SLOTS;
    for (int i = threadIdx.x; i < SLOTS; i += blockDim.x) {
        lkey[i] = EMPTY_KEY;
        cA[i] = 0;
        cB[i] = 0;
    }
    if (threadIdx.x == 0) blk_cnt = 0;
    __syncthreads();
    const uint32_t nsub = M.range / M.cpi_range;
    for (int p = 0; p < M.n_src; p++) {
        const int inA = (int)((M.maskA >> p) & 1);
        const int inB = (int)((M.maskB >> p) & 1);
        auto fold = [&](int64_t key, uint64_t w0) {
            if (key == EMPTY_KEY) return;
            uint32_t h = (uint32_t)hash64((uint64_t)key * 0x9e3779b1u) &
                         (SLOTS - 1);
            int64_t slot = -1;
            for (int pr = 0; pr < SLOTS && slot < 0; pr++) {
                uint32_t sidx = (h + pr) & (SLOTS - 1);
                int64_t k = lkey[sidx];
                if (k == key) {
                    slot = sidx;
                } else if (k == EMPTY_KEY) {
                    int64_t old = (int64_t)atomicCAS(
                        (unsigned long long *)&lkey[sidx],
                        (unsigned long long)EMPTY_KEY,
                        (unsigned long long)key);
                    if (old == EMPTY_KEY || old == key) slot = sidx;
                }
            }
            if (slot < 0) { *M.ring.err = ERR_MF_OVERFLOW; return; }
            if (inA)
                atomicAdd((unsigned long long *)&cA[slot],
                          (unsigned long long)w0);
            if (inB)
                atomicAdd((unsigned long long *)&cB[slot],
                          (unsigned long long)w0);
        };
        for (uint32_t j = 0; j < nsub; j++) {
            uint32_t seg = blockIdx.x * nsub + j;
            const uint32_t n_e = M.cpi_cnt[p][seg];
            const uint64_t *ent = M.cpi_entries[p] +
                                  (size_t)seg * M.cpi_range * 2;
            for (uint32_t t = threadIdx.x; t < n_e; t += blockDim.x) {
                ulonglong2 e = ((const ulonglong2 *)ent)[t];
                fold((int64_t)e.x, (uint64_t)e.y);
            }
        }
    }
    __syncthreads();
    unsigned int mine = 0;
    for (int i = threadIdx.x; i < SLOTS; i += blockDim.x)
        if (lkey[i] != EMPTY_KEY)
            mine += (cA[i] > 0) + (cB[i] > 0);
    for (int off = 32; off; off >>= 1)
        mine += (unsigned)__shfl_down((int)mine, off, 64);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(&blk_cnt, mine);
    __syncthreads();
    if (threadIdx.x == 0) {
        blk_base = blk_cnt ? atomicAdd(M.n_out,
                                       (unsigned long long)blk_cnt)
                           : 0;
        if (M.accum && blk_cnt)
            atomicAdd(M.accum, (unsigned long long)blk_cnt);
        blk_cnt = 0;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < SLOTS; i += blockDim.x) {
        int64_t key = lkey[i];
        if (key == EMPTY_KEY) continue;
        for (int w = 0; w < 2; w++) {
            uint64_t c = w ? cB[i] : cA[i];
            if (!c) continue;
            int64_t r = (int64_t)(blk_base + atomicAdd(&blk_cnt, 1u));
            int col = 0;
            if (M.n_keys) M.out[col++][r] = key;
            M.out[col++][r] = (int64_t)c;
            M.out[col++][r] = (int64_t)(w ? M.wsB : M.wsA);
            M.out[col++][r] = (int64_t)(w ? M.weB : M.weA);
            M.out[col][r] = (int64_t)((w ? M.weB : M.weA) - 1);
        }
    }
    /* special (key == sentinel) entries */
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        for (int w = 0; w < 2; w++) {
            uint64_t mask = w ? M.maskB : M.maskA;
            uint64_t sum = 0;
            int any = 0;
            for (int p = 0; p < M.n_src; p++) {
                if (!((mask >> p) & 1)) continue;
                uint32_t pp = M.src[p];
                if (!M.ring.spec_used[pp]) continue;
                any = 1;
                /* dual is COUNT-shaped only: na == 1, stride 2 words */
                sum += M.ring.spec_state[(size_t)pp * 2];
            }
            if (!any) continue;
            int64_t r = (int64_t)atomicAdd(M.n_out, 1ULL);
            if (M.accum) atomicAdd(M.accum, 1ULL);
            int col = 0;
            if (M.n_keys) M.out[col++][r] = EMPTY_KEY;
            M.out[col++][r] = (int64_t)sum;
            M.out[col++][r] = (int64_t)(w ? M.wsB : M.wsA);
            M.out[col++][r] = (int64_t)(w ? M.weB : M.weA);
            M.out[col][r] = (int64_t)((w ? M.weB : M.weA) - 1);
        }
    }
}

template __global__ void k_merge_dual<2048>(MergeDualArgs);

/* restore checkpointed partial states: insert raw state rows into a pane. */
struct RestoreArgs {
    const int64_t *key_col;           /* null when unkeyed */
    const int64_t *scols[2 * AMD_MAX_AGGS];
    int32_t  swords[AMD_MAX_AGGS];    /* 1 or 2 (AVG) words per agg */
    int64_t  n_rows;
    uint32_t pane;
    DeviceRing ring;
    AggSpec agg;
};

__global__ void __launch_bounds__(256)
k_restore(RestoreArgs R) {
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         i < R.n_rows; i += stride) {
        int64_t key = R.key_col ? R.key_col[i] : 0;
        uint64_t enc[2 * AMD_MAX_AGGS];
        int c = 0;
        for (int a = 0; a < R.agg.n_aggs; a++) {
            int64_t w0 = R.scols[c][i];
            enc[2 * a] = enc_word(R.agg.op[a], R.agg.isf[a], w0);
            if (R.agg.op[a] == AMD_AGG_AVG)
                enc[2 * a + 1] = (uint64_t)R.scols[c + 1][i];
            c += R.swords[a];
        }
        uint32_t p = R.pane;
        uint64_t *st;
        if (key == EMPTY_KEY) {
            atomicExch(&R.ring.spec_used[p], 1u);
            st = R.ring.spec_state + (size_t)p * R.agg.n_aggs * 2;
        } else {
            int64_t *keys = R.ring.keys + (size_t)p * R.ring.C;
            int64_t s = table_upsert(keys, R.ring.C, key, R.ring.err);
            if (s < 0) continue;
            st = R.ring.state +
                 ((size_t)p * R.ring.C + (size_t)s) * R.agg.n_aggs * 2;
        }
        atomic_merge(st, enc, R.agg);
    }
}

/* clear one pane's scalar metadata in a single launch (replaces four
 * 4-8 B memset launches at retire) */
__global__ void k_retire_meta(uint64_t *tag, uint32_t *spec_used,
                              uint64_t *spec_state, int na2) {
    *tag = EMPTY_TAG;
    *spec_used = 0;
    for (int w = 0; w < na2; w++) spec_state[w] = 0;
}

/* K8: shuffle partition ids -- hash(key) -> contiguous range owner,
 * matching server_for_hash (crates/arroyo-types/src/lib.rs:640-647). */
__global__ void __launch_bounds__(256)
k_partition(const int64_t *keys, int64_t n, uint32_t n_parts,
            uint32_t *part_ids, unsigned long long *counts) {
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    uint64_t range = n_parts > 1 ? (~0ULL / n_parts) + 1 : 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         i < n; i += stride) {
        uint32_t p = n_parts > 1
                         ? (uint32_t)(hash64((uint64_t)keys[i]) / range)
                         : 0;
        part_ids[i] = p;
        atomicAdd(&counts[p], 1ULL);
    }
}

/* scatter rows into per-partition contiguous segments (offsets = exclusive
 * prefix sum of counts, computed on host over <=8 entries). */
__global__ void __launch_bounds__(256)
k_scatter(const uint32_t *part_ids, unsigned long long *cursors,
          const int64_t *const in0, const int64_t *const in1,
          const int64_t *const in2, int64_t *out0, int64_t *out1,
          int64_t *out2, int64_t n) {
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         i < n; i += stride) {
        int64_t d = (int64_t)atomicAdd(&cursors[part_ids[i]], 1ULL);
        out0[d] = in0[i];
        if (in1) out1[d] = in1[i];
        if (in2) out2[d] = in2[i];
    }
}

/* ------------------------------------------------------------------ */
/* host side: operator handle + state machine                          */

/* update kernel of an operator (ARROYO_AMD_UPD=lds|batch|tile) */
enum UpdKind {
    UPD_LDS,    /* k_update_lds_vec / k_update_lds: every shape; the only
                   kind for anything but keyed single-COUNT */
    UPD_BATCH,  /* k_update_batch_n: keyed single-COUNT, kept as the
                   documented comparison for the tile kernel */
    UPD_TILE,   /* k_update_tile: keyed single-COUNT, its default */
};

struct GpuOp : OpBase {
    AmdWindowConfig cfg;
    AggSpec agg;
    int n_in_cols;       /* n_keys + n_value_cols + 1 */
    int out_cols;
    uint64_t width, slide;

    DeviceRing ring;
    int64_t  *m_keys;
    /* m_state/m_fill/m_spec_used/m_spec_state/d_n_out live in ONE
     * contiguous zero-blob so a fire clears them with a single memset */
    uint64_t *m_zero_blob;
    size_t    m_zero_bytes;
    uint64_t *m_state;
    uint32_t *m_spec_used;
    uint64_t *m_spec_state;
    uint32_t CM;

    int64_t *d_out[16];       /* device output columns, CM+1 rows each */
    int n_out_alloc;
    unsigned long long *d_n_out;
    unsigned long long *d_emitted;  /* running device-side emitted rows */
    unsigned long long *d_fire_cur; /* 64 rotating fused-fire row cursors:
                                       an 8-byte memset launch per fire
                                       (~4 us on the fire stream) becomes
                                       one 512 B memset per 64 fires */
    unsigned long long *d_fire_cur2;  /* fstream2's own ring (a shared
                                         ring's wrap memset would race the
                                         other stream's running merge) */
    uint64_t fire_seq, fire_seq2;
    /* row cursor of the latest fire into d_out ([0]) / d_out2 ([1]); read
     * back only by arroyo_amd_last_emission */
    unsigned long long *last_cur[2];
    int64_t out_rows_cap;

    /* host-accumulated emission (emit_to_host) */
    std::vector<std::vector<int64_t>> host_out;

    /* fire path (pane close -> cpi build -> merge -> retire) runs on its
     * own stream, overlapping the NEXT periods' update kernels: both are
     * latency-bound (update 87.5% memory-parked, merge ~470 GB/s) so
     * co-resident waves raise aggregate memory-level parallelism.  Safe
     * because the late-row filter guarantees no update launched after
     * watermark W writes a pane W's fires read.  fstream == stream when
     * ARROYO_AMD_FIRE_STREAM=0 (serial debug mode). */
    hipStream_t fstream;
    /* second fire stream: a period's two window merges are independent
     * read-only scans of overlapping closed panes, both latency-bound, so
     * they run concurrently (alternating streams); retires wait on both */
    hipStream_t fstream2;
    hipEvent_t ev_f1, ev_f2, ev_cpi;
    int f2_dirty;             /* fstream2 has unwaited merge work */
    uint64_t fire_alt;
    int64_t *d_out2[16];      /* fstream2's output columns (row ranges of
                                 concurrent merges must not collide) */
    int own_fstream;
    hipEvent_t ev_gate;       /* updates-done gate the fire stream waits on */
    hipEvent_t ev_tail[4];    /* per-group fire-tail ring: bounds the fire
                                 stream's lag to 4 groups << R/2 periods, so
                                 a ring slot's retire always completes
                                 before the slot's bin comes around again */
    uint64_t fire_group;
    std::vector<uint32_t> retire_pend;  /* slots awaiting the tag clear */
    /* deferred fires within one batched watermark call, so consecutive
     * windows can be paired into k_merge_dual (see the kernel's doc) */
    struct PendFire { std::vector<uint32_t> src; uint64_t ws, we; };
    std::vector<PendFire> pend_fires;
    std::vector<std::pair<uint32_t, uint64_t>> pend_retires;
    int defer_fires;
    int spin;                 /* busy-wait host syncs (ARROYO_AMD_SPIN) */
    hipEvent_t ev_sync;       /* status-copy completion (spin target) */
    /* epoch pipeline (mark_epoch / handle_watermarks_epoch): per-epoch
     * pinned status snapshots so the harness can submit the NEXT period
     * before folding this one's watermarks */
    uint64_t *h_epoch[2];
    hipEvent_t ev_epoch[2];
    int epoch_head, epoch_cnt;
    int fire_lag;             /* groups of slack before the lag wait (<=3;
                                 reuse distance R/bins-per-group >> this) */
    std::vector<uint64_t> retired_bin;  /* [R] bin whose async retire may
                                           not yet show in d_status */
    /* pinned host staging for host-memory process_batch calls:
     * key?, vcols..., ts (restore: key?, states...) */
    Staging stg;

    /* one contiguous device status block [err, min_bin, tags[R]] mirrored
     * into pinned host memory: ONE copy + ONE sync per watermark instead of
     * three separate round trips (check_device_error + min_bin +
     * sync_open_panes were ~60 us of host latency per watermark) */
    uint64_t *d_status;
    uint64_t *h_status;   /* pinned */

    /* host state machine (sliding_aggregating_window.rs:63-73) */
    int state;               /* 0 NoData 1 OnlyBufferedData 2 InMemoryData */
    uint64_t earliest, next_start;
    int has_wm; uint64_t wm;
    std::map<uint64_t, uint32_t> open;    /* bin -> ring slot (host view) */
    std::map<uint64_t, uint32_t> closed;  /* bin -> ring slot (tiered) */
    std::set<uint64_t> table_bins;        /* ExpiringTimeKeyView keys */

    UpdKind upd_kind;
    /* closed-pane index (see CpiBuildArgs) */
    uint64_t *cpi_entries;      /* [R][NR][cpi_range][cpi_ew] */
    uint32_t *cpi_cnt;          /* [R][NR] */
    int cpi_ew;
    uint32_t cpi_range;         /* build granularity (<= mf_range) */
    uint32_t mf_range;          /* fused-merge home-range size (fixed) */
    uint32_t cpi_nr;            /* C / mf_range */
    std::vector<char> cpi_ready;
    /* multi-column keys: device dictionary (see k_dict_encode) */
    int mk;                     /* 1 when cfg.n_keys >= 2 */
    int64_t *d_dict_digest;
    int64_t *d_dict_keys;
    uint32_t *d_dict_ready;
    uint32_t dict_D;
    int64_t *d_keyid_in;
    int64_t keyid_in_cap;
    int64_t *d_keyid_out;
    /* update-launch knobs, read once at create */
    int force_blocks;         /* ARROYO_AMD_BLOCKS: grid size, 0 = computed */
    int bq;                   /* ARROYO_AMD_BQ: rows per thread per iteration
                                 of the batch and tile kernels: 8, 12 or 16 */
    int pblocks;              /* ARROYO_AMD_PBLOCKS: batch grid cap / tile
                                 block budget */
    int pblocks_set;          /* ... was given (else the tile budget is
                                 tile_resident) */
    int tile_s;               /* ARROYO_AMD_TILE_S: tile span, 0 = computed */
    int tile_resident;        /* k_update_tile<bq> blocks the device holds at
                                 once; queried at the first tile launch */
    int use_events;
    /* perf counters for bench; a fixed pool of reusable event pairs samples
     * a subset of launches (create/destroy per launch was host overhead) */
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pool;
    std::vector<int> ev_inflight;  /* indices into ev_pool */
    double   update_kernel_ms;     /* sum over SAMPLED launches */
    int64_t  sampled_launches;
    int64_t  update_rows;
    int64_t  launches;
    int64_t  emitted_device_rows;
};

#define EV_POOL 64

/* fold finished sampled-launch timings; block=0 leaves unfinished pairs
 * inflight (the epoch-pipelined fold must not wait on the NEXT period's
 * update kernels), block=1 (perf/destroy) drains everything */
static void harvest_events(GpuOp *o, int block) {
    std::vector<int> keep;
    for (int idx : o->ev_inflight) {
        if (!block &&
            hipEventQuery(o->ev_pool[idx].second) == hipErrorNotReady) {
            keep.push_back(idx);
            continue;
        }
        hipEventSynchronize(o->ev_pool[idx].second);
        float ms = 0;
        hipEventElapsedTime(&ms, o->ev_pool[idx].first,
                            o->ev_pool[idx].second);
        o->update_kernel_ms += ms;
        o->sampled_launches++;
    }
    (void)hipGetLastError();   /* clear NotReady sticky */
    o->ev_inflight = std::move(keep);
}

/* order the fire stream after every update launched so far (one event) */
static int gate_fire(GpuOp *o) {
    if (o->fstream == o->stream) return 0;
    HIP_CHECK(o, hipEventRecord(o->ev_gate, o->stream));
    HIP_CHECK(o, hipStreamWaitEvent(o->fstream, o->ev_gate, 0));
    HIP_CHECK(o, hipStreamWaitEvent(o->fstream2, o->ev_gate, 0));
    return 0;
}

/* record this watermark group's fire tail (retires included) */
static int fire_tail(GpuOp *o) {
    if (o->fstream == o->stream) return 0;
    /* the tail must cover BOTH fire streams (odd merges + cpi builds) */
    HIP_CHECK(o, hipEventRecord(o->ev_f2, o->fstream2));
    HIP_CHECK(o, hipStreamWaitEvent(o->fstream, o->ev_f2, 0));
    o->f2_dirty = 0;
    HIP_CHECK(o, hipEventRecord(o->ev_tail[o->fire_group & 3], o->fstream));
    o->fire_group++;
    return 0;
}

/* bound the fire stream's lag: at each group's fold (called AFTER the
 * group's own update launches were enqueued, so the previous group's
 * fires still overlap them), order all later main-stream work after the
 * PREVIOUS group's fire tail.  Slot reuse is bin-deterministic
 * (p = q & (R-1)) and a slot's retire is enqueued width/slide bins after
 * its close, so the reuse claim comes >= (R - width/slide - fused bins)
 * bins after the retire's group -- a lag bound of one group keeps the
 * claim strictly after the retire for every tested R (a 4-group bound
 * measurably raced at ring_panes=16 with large pane memsets: loud
 * ERR_RING_CONFLICT, never corruption). */
static int bound_fire_lag(GpuOp *o) {
    if (o->fstream == o->stream ||
        o->fire_group < (uint64_t)o->fire_lag) return 0;
    HIP_CHECK(o, hipStreamWaitEvent(
                     o->stream,
                     o->ev_tail[(o->fire_group - o->fire_lag) & 3], 0));
    return 0;
}

static int ring_retire_flush(GpuOp *o);

/* plane clears only; the tag is cleared LAST by ring_retire_flush (one
 * kernel for the whole batch of retires), via stream order */
static int ring_retire_planes(GpuOp *o, uint32_t slot, uint64_t bin) {
    size_t na = o->agg.n_aggs;
    if (o->f2_dirty) {   /* pane clears must follow fstream2's merges */
        HIP_CHECK(o, hipStreamWaitEvent(o->fstream, o->ev_f2, 0));
        o->f2_dirty = 0;
    }
    if (slot < o->cpi_ready.size()) o->cpi_ready[slot] = 0;
    if (slot < o->retired_bin.size()) o->retired_bin[slot] = bin;
    int blocks = (int)((o->ring.C + 255) / 256);
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(k_retire_all, dim3(blocks), dim3(256), 0, o->fstream,
                       o->ring.keys + (size_t)slot * o->ring.C,
                       o->ring.state + (size_t)slot * o->ring.C * na * 2,
                       (int64_t)o->ring.C, (int)(na * 2));
    HIP_CHECK(o, hipGetLastError());
    o->retire_pend.push_back(slot);
    if ((int)o->retire_pend.size() >= 8) return ring_retire_flush(o);
    return 0;
}

static int ring_retire_flush(GpuOp *o) {
    if (o->retire_pend.empty()) return 0;
    RetireTagsArgs A = {};
    A.tag = o->ring.tag;
    A.spec_used = o->ring.spec_used;
    A.spec_state = o->ring.spec_state;
    A.na2 = (int)(o->agg.n_aggs * 2);
    A.n = (int)o->retire_pend.size();
    for (int i = 0; i < A.n; i++) A.slot[i] = o->retire_pend[i];
    o->retire_pend.clear();
    hipLaunchKernelGGL(k_retire_tags, dim3(1), dim3(1), 0, o->fstream, A);
    HIP_CHECK(o, hipGetLastError());
    return 0;
}

static int ring_retire(GpuOp *o, uint32_t slot, uint64_t bin) {
    if (ring_retire_planes(o, slot, bin)) return 1;
    return ring_retire_flush(o);
}

static int flush_staged(GpuOp *o);

/* compact a freshly-closed pane into its home-range-grouped index */
static int cpi_build(GpuOp *o, uint32_t slot) {
    if (!o->cpi_entries) return 0;
    size_t na = o->agg.n_aggs;
    CpiBuildArgs A = {};
    A.keys = o->ring.keys + (size_t)slot * o->ring.C;
    A.state = o->ring.state + (size_t)slot * o->ring.C * na * 2;
    A.C = o->ring.C;
    A.ew = o->cpi_ew;
    A.na = (int32_t)na;
    A.range = o->cpi_range;
    A.nr = o->cpi_nr;
    A.cnt = o->cpi_cnt + (size_t)slot * o->cpi_nr;
    A.entries = o->cpi_entries + (size_t)slot * o->ring.C * o->cpi_ew;
    A.err = o->ring.err;
    hipLaunchKernelGGL(k_cpi_build, dim3(o->cpi_nr), dim3(256), 0,
                       o->fstream2, A);
    HIP_CHECK(o, hipGetLastError());
    if (o->fstream2 != o->fstream)
        HIP_CHECK(o, hipEventRecord(o->ev_cpi, o->fstream2));
    o->cpi_ready[slot] = 1;
    return 0;
}

API void *arroyo_amd_create(const AmdWindowConfig *cfg) {
    if (!cfg || cfg->n_aggs < 1 || cfg->n_aggs > AMD_MAX_AGGS ||
        cfg->n_keys < 0 || cfg->n_keys > 4 || cfg->width_nanos == 0 ||
        cfg->n_value_cols > 4) {
        snprintf(g_create_err, sizeof g_create_err, "invalid config");
        return nullptr;
    }
    for (int i = 0; i < cfg->n_aggs; i++)
        if (cfg->agg_ops[i] >= AMD_AGG_MEDIAN &&
            cfg->agg_ops[i] <= AMD_AGG_MAX_RETRACT) {
            snprintf(g_create_err, sizeof g_create_err,
                     "invalid config: aggregate op %d is updating-aggregate "
                     "only", cfg->agg_ops[i]);
            return nullptr;
        }
    if (!cfg->is_tumbling && cfg->slide_nanos != 0 &&
        cfg->width_nanos % cfg->slide_nanos != 0) {
        /* the reference's planner rejects this (arroyo-planner/src/lib.rs
         * :644: "hop() width currently must be a multiple of slide") */
        snprintf(g_create_err, sizeof g_create_err,
                 "hop() width must be a multiple of slide");
        return nullptr;
    }
    if (!cfg->is_tumbling && cfg->slide_nanos == 0) {
        snprintf(g_create_err, sizeof g_create_err,
                 "sliding window needs slide > 0");
        return nullptr;
    }
    GpuOp *o = new GpuOp();
    o->cfg = *cfg;
    /* read before the allocation block: d_out2 existence depends on it */
    o->own_fstream = 1;
    if (const char *ev = getenv("ARROYO_AMD_FIRE_STREAM"))
        o->own_fstream = atoi(ev) != 0;
    /* hop(x, x) is a tumble window (arroyo-planner/src/lib.rs:649-651) */
    if (!o->cfg.is_tumbling && o->cfg.slide_nanos == o->cfg.width_nanos)
        o->cfg.is_tumbling = 1;
    if (o->cfg.is_tumbling) o->cfg.slide_nanos = o->cfg.width_nanos;
    o->width = o->cfg.width_nanos;
    o->slide = o->cfg.slide_nanos;
    o->agg.n_aggs = cfg->n_aggs;
    for (int i = 0; i < cfg->n_aggs; i++) {
        o->agg.op[i] = cfg->agg_ops[i];
        o->agg.col[i] = cfg->agg_col[i];
        o->agg.isf[i] = cfg->agg_col[i] >= 0 &&
                        cfg->val_is_f64[cfg->agg_col[i]];
    }
    o->n_in_cols = cfg->n_keys + cfg->n_value_cols + 1;
    o->out_cols = cfg->n_keys + cfg->n_aggs + 3;
    int raw_cols = cfg->n_keys + 1;
    for (int i = 0; i < cfg->n_aggs; i++)
        raw_cols += (cfg->agg_ops[i] == AMD_AGG_AVG) ? 2 : 1;
    o->n_out_alloc = o->out_cols > raw_cols ? o->out_cols : raw_cols;
    o->ring.C = 1u << cfg->log2_capacity;
    o->ring.R = cfg->ring_panes ? cfg->ring_panes : 64;
    o->CM = o->ring.C * 2;
    o->state = 0;
    o->force_blocks = 0;
    if (const char *e = getenv("ARROYO_AMD_BLOCKS")) o->force_blocks = atoi(e);
    o->bq = 8;
    if (const char *e = getenv("ARROYO_AMD_BQ")) o->bq = atoi(e);
    o->bq = o->bq >= 16 ? 16 : o->bq >= 12 ? 12 : 8;
    o->pblocks = 2048;
    o->pblocks_set = 0;
    if (const char *e = getenv("ARROYO_AMD_PBLOCKS")) {
        o->pblocks = atoi(e);
        o->pblocks_set = 1;
    }
    o->tile_s = 0;
    if (const char *e = getenv("ARROYO_AMD_TILE_S"))
        if (atoi(e) > 0) o->tile_s = atoi(e);
    o->tile_resident = 0;
    o->use_events = 1;
    if (const char *e = getenv("ARROYO_AMD_EVENTS")) o->use_events = atoi(e);

    if (hipSetDevice(cfg->device) != hipSuccess) {
        snprintf(g_create_err, sizeof g_create_err,
                 "hipSetDevice(%d) failed: no HIP device (the arroyo-amd "
                 "product path requires a GPU; it never falls back to CPU)",
                 cfg->device);
        delete o;
        return nullptr;
    }
    size_t na = o->agg.n_aggs;
    /* update kernel: the keyed single-COUNT shape (the q5 headline) takes
     * the tile kernel by default and may be switched to "batch" or "lds";
     * every other shape always takes the LDS-staged kernel.  An unknown
     * value leaves the shape's default. */
    bool count_shape = (o->cfg.n_keys == 1 && o->agg.n_aggs == 1 &&
                        o->agg.op[0] == AMD_AGG_COUNT);
    o->upd_kind = count_shape ? UPD_TILE : UPD_LDS;
    if (const char *ev = getenv("ARROYO_AMD_UPD")) {
        if (!strcmp(ev, "lds")) o->upd_kind = UPD_LDS;
        else if (count_shape && !strcmp(ev, "batch")) o->upd_kind = UPD_BATCH;
        else if (count_shape && !strcmp(ev, "tile")) o->upd_kind = UPD_TILE;
    }
    OP_ALLOC(o, o->ring.keys, (size_t)o->ring.R * o->ring.C * 8, 0xFF);
    OP_ALLOC(o, o->ring.state, (size_t)o->ring.R * o->ring.C * na * 16, 0);
    /* status block [err, min_bin, tags[R]]: err 0, the rest all-0xFF */
    OP_ALLOC(o, o->d_status, (2 + (size_t)o->ring.R) * 8, 0xFF);
    o->ring.err = (int *)o->d_status;
    o->ring.min_bin = o->d_status + 1;
    o->ring.tag = o->d_status + 2;
    OP_TRY(o, "d_status", hipMemset(o->ring.err, 0, 4));
    OP_TRY(o, "h_status",
           o->pinned_alloc(o->h_status, (2 + (size_t)o->ring.R) * 8));
    OP_ALLOC(o, o->ring.spec_used, (size_t)o->ring.R * 4, 0);
    OP_ALLOC(o, o->ring.spec_state, (size_t)o->ring.R * na * 16, 0);
    OP_ALLOC(o, o->m_keys, (size_t)o->CM * 8, 0xFF);
    o->m_zero_bytes = (size_t)o->CM * na * 16 + 8 + na * 16 + 8;
    OP_ALLOC(o, o->m_zero_blob, o->m_zero_bytes, 0);
    o->m_state = o->m_zero_blob;
    o->m_spec_used =
        (uint32_t *)(o->m_zero_blob + (size_t)o->CM * na * 2);
    o->m_spec_state = o->m_zero_blob + (size_t)o->CM * na * 2 + 1;
    o->d_n_out = (unsigned long long *)(o->m_spec_state + na * 2);
    o->out_rows_cap = (int64_t)o->CM + 1;
    for (int i = 0; i < o->n_out_alloc; i++)
        OP_ALLOC(o, o->d_out[i], (size_t)o->out_rows_cap * 8);
    if (o->own_fstream)
        for (int i = 0; i < o->n_out_alloc; i++)
            OP_ALLOC(o, o->d_out2[i], (size_t)o->out_rows_cap * 8);
    OP_ALLOC(o, o->d_emitted, 8, 0);
    OP_ALLOC(o, o->d_fire_cur, 64 * 8, 0);
    OP_ALLOC(o, o->d_fire_cur2, 64 * 8, 0);
    /* fused-merge home range fixed at create (CPI grouping depends on it) */
    o->mf_range = MF_RANGE;
    if (const char *ev = getenv("ARROYO_AMD_MF_RANGE"))
        o->mf_range = (uint32_t)atoi(ev);
    if (o->mf_range < 2) o->mf_range = 2;
    if (o->mf_range > o->ring.C) o->mf_range = o->ring.C;
    while (o->mf_range & (o->mf_range - 1)) o->mf_range &= o->mf_range - 1;
    /* build granularity: small enough sub-ranges that the build grid can
     * hide memory latency (512 WGs was 2 waves/SIMD and 30 us), but not
     * so small that the merge's per-segment scan idles most of its
     * threads (the sweep: 512 > 256 > 128; whole-job 23.8/22.3/18.1 G) */
    o->cpi_range = o->mf_range > 512 ? 512 : o->mf_range;
    if (const char *ev = getenv("ARROYO_AMD_CPI_RANGE")) {
        o->cpi_range = (uint32_t)atoi(ev);
        if (o->cpi_range < 2) o->cpi_range = 2;
        if (o->cpi_range > o->mf_range) o->cpi_range = o->mf_range;
        while (o->cpi_range & (o->cpi_range - 1))
            o->cpi_range &= o->cpi_range - 1;
    }
    o->cpi_nr = o->ring.C / o->cpi_range;
    if (na <= MF_MAX_AGGS && !o->cfg.is_tumbling &&
        o->cpi_nr <= CPI_MAX_NR) {
        int use_cpi = 1;
        if (const char *ev = getenv("ARROYO_AMD_CPI")) use_cpi = atoi(ev);
        if (use_cpi) {
            o->cpi_ew = (na == 1 && o->agg.op[0] != AMD_AGG_AVG)
                            ? 2 : (int)(1 + 2 * na);
            OP_ALLOC(o, o->cpi_entries,
                     (size_t)o->ring.R * o->ring.C * o->cpi_ew * 8);
            OP_ALLOC(o, o->cpi_cnt, (size_t)o->ring.R * o->cpi_nr * 4);
        }
    }
    o->cpi_ready.assign(o->ring.R, 0);
    o->mk = o->cfg.n_keys >= 2;
    if (o->mk) {
        /* dictionary 4x the pane table; ids must stay stable, so no
         * eviction — exhaustion is a loud ERR_DICT_FULL */
        o->dict_D = o->ring.C << 2;
        OP_ALLOC(o, o->d_dict_digest, (size_t)o->dict_D * 8, 0xFF);
        OP_ALLOC(o, o->d_dict_keys, (size_t)o->dict_D * o->cfg.n_keys * 8);
        OP_ALLOC(o, o->d_dict_ready, (size_t)o->dict_D * 4, 0);
        OP_ALLOC(o, o->d_keyid_out, (size_t)o->out_rows_cap * 8);
    }
    o->fire_seq = o->fire_seq2 = 0;
    /* the update stream paces the period: give it scheduler priority over
     * the fire streams so its blocks win the CU race (fires have slack) */
    int pr_lo = 0, pr_hi = 0;
    OP_TRY(o, "stream priority range",
           hipDeviceGetStreamPriorityRange(&pr_lo, &pr_hi));
    OP_TRY(o, "stream", o->own_stream(o->stream, hipStreamCreateWithPriority(
                            &o->stream, hipStreamNonBlocking, pr_hi)));
    if (o->own_fstream) {
        /* ARROYO_AMD_FIRE_CUS=N confines both fire streams to the last N
         * CUs so update wavefronts own the rest (hard partition via CU
         * mask); 0/unset = share the whole chip under priorities */
        int fire_cus = 0;
        if (const char *ev = getenv("ARROYO_AMD_FIRE_CUS"))
            fire_cus = atoi(ev);
        if (fire_cus > 0 && fire_cus < 256) {
            uint32_t mask[8] = {};
            for (int b = 256 - fire_cus; b < 256; b++)
                mask[b / 32] |= 1u << (b % 32);
            for (hipStream_t *fs : {&o->fstream, &o->fstream2})
                OP_TRY(o, "fire stream",
                       o->own_stream(*fs, hipExtStreamCreateWithCUMask(
                                              fs, 8, mask)));
        } else {
            for (hipStream_t *fs : {&o->fstream, &o->fstream2})
                OP_TRY(o, "fire stream",
                       o->own_stream(*fs,
                                     hipStreamCreateWithPriority(
                                         fs, hipStreamNonBlocking, pr_lo)));
        }
        for (hipEvent_t *ev : {&o->ev_gate, &o->ev_f1, &o->ev_f2, &o->ev_cpi,
                               &o->ev_tail[0], &o->ev_tail[1], &o->ev_tail[2],
                               &o->ev_tail[3]})
            OP_TRY(o, "fire event",
                   o->event_create(ev, hipEventDisableTiming));
    } else {
        o->fstream = o->stream;
        o->fstream2 = o->stream;
    }
    o->f2_dirty = 0;
    o->fire_alt = 0;
    o->fire_group = 0;
    o->spin = 1;
    if (const char *ev = getenv("ARROYO_AMD_SPIN")) o->spin = atoi(ev) != 0;
    OP_TRY(o, "ev_sync", o->event_create(&o->ev_sync, hipEventDisableTiming));
    for (int i = 0; i < 2; i++) {
        OP_TRY(o, "h_epoch",
               o->pinned_alloc(o->h_epoch[i], (2 + (size_t)o->ring.R) * 8));
        OP_TRY(o, "ev_epoch",
               o->event_create(&o->ev_epoch[i], hipEventDisableTiming));
    }
    o->epoch_head = o->epoch_cnt = 0;
    /* 2 groups of slack won the sweep (lag 1 throttles updates behind a
     * slow fire group, -6%; the reuse distance R/bins-per-group leaves
     * >= 2 periods of margin at the bench shapes, and a violated margin
     * is a loud ring-conflict, not corruption) */
    o->fire_lag = 2;
    if (const char *ev = getenv("ARROYO_AMD_FIRE_LAG")) {
        o->fire_lag = atoi(ev);
        if (o->fire_lag < 1) o->fire_lag = 1;
        if (o->fire_lag > 3) o->fire_lag = 3;
    }
    o->retired_bin.assign(o->ring.R, EMPTY_TAG);
    /* pinned staging: 1M rows; enough columns for input batches and for
     * restore's raw-state batches */
    OP_TRY_MSG(o, "staging alloc failed",
               o->stg.alloc(o, o->n_in_cols > raw_cols - 1 ? o->n_in_cols
                                                       : raw_cols - 1,
                        1 << 20));
    o->host_out.resize(o->out_cols);
    return o;
}

API const char *arroyo_amd_last_error(void *h) {
    return h ? ((GpuOp *)h)->err_msg : g_create_err;
}

/* 16 B vector loads need a row pair and 16 B-aligned ts/key columns */
static bool cols_vec_ok(const UpdateArgs &A) {
    return A.n_rows >= 2 && ((uintptr_t)A.ts_col & 15) == 0 &&
           ((uintptr_t)A.key_col & 15) == 0;   /* null (unkeyed) passes */
}

/* UPD_LDS: two rows per thread when the columns allow it, else one */
static void launch_lds(GpuOp *o, const UpdateArgs &A) {
    bool vec = cols_vec_ok(A);
    int64_t units = vec ? (A.n_rows + 1) / 2 : A.n_rows;
    int64_t want = (units + 255) / 256;
    /* grid-sweep optima: 640 blocks at ~0.5M units (1M-row launches), 896
     * at ~1M units (2M-row fused launches).  Fewer blocks -> fewer
     * same-key flush contenders on the global table; more -> better tail
     * occupancy at larger launches. */
    int cap = units >= (640 << 10) ? 896 : 640;
    int blocks = (int)(want > cap ? cap : (want < 1 ? 1 : want));
    if (o->force_blocks > 0) blocks = o->force_blocks;
    size_t shmem = (size_t)LDS_SLOTS * o->agg.n_aggs * 16;
    bool count_only = o->agg.n_aggs == 1 && o->agg.op[0] == AMD_AGG_COUNT;
    if (!vec)
        hipLaunchKernelGGL(k_update_lds, dim3(blocks), dim3(256), shmem,
                           o->stream, A);
    else if (count_only)
        hipLaunchKernelGGL((k_update_lds_vec<LDS_SLOTS, true>), dim3(blocks),
                           dim3(256), shmem, o->stream, A);
    else
        hipLaunchKernelGGL((k_update_lds_vec<LDS_SLOTS, false>), dim3(blocks),
                           dim3(256), shmem, o->stream, A);
}

/* the batch and tile kernels skip the last n_rows % bq rows; finish them
 * with a tiny scalar launch (same parity) */
static void launch_batch_tail(GpuOp *o, const UpdateArgs &A) {
    int64_t tail = A.n_rows % o->bq;
    if (!tail) return;
    UpdateArgs T = A;
    T.key_col = A.key_col + (A.n_rows - tail);
    T.ts_col = A.ts_col + (A.n_rows - tail);
    T.n_rows = tail;
    hipLaunchKernelGGL(k_update_batch_scalar, dim3(1), dim3(64), 0, o->stream,
                       T);
}

/* UPD_BATCH: grid-stride k_update_batch_n<bq>; the scalar kernel when the
 * columns cannot be vector-loaded (UPD_TILE shares that fallback) */
static void launch_batch(GpuOp *o, const UpdateArgs &A) {
    bool vec = cols_vec_ok(A);
    int64_t units = vec ? (A.n_rows + 1) / 4 : A.n_rows;
    int64_t want = (units + 255) / 256;
    int blocks = (int)(want > o->pblocks ? o->pblocks : (want < 1 ? 1 : want));
    if (o->force_blocks > 0) blocks = o->force_blocks;
    if (!vec) {
        hipLaunchKernelGGL(k_update_batch_scalar, dim3(blocks), dim3(256), 0,
                           o->stream, A);
        return;
    }
    auto kern = k_update_batch_n<8>;
    if (o->bq == 16) kern = k_update_batch_n<16>;
    else if (o->bq == 12) kern = k_update_batch_n<12>;
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), 0, o->stream, A);
    launch_batch_tail(o, A);
}

/* UPD_TILE: contiguous spans: block b owns sub-tiles [b*S, (b+1)*S) of
 * 256*bq rows.  The block budget only sets the span length, so locality
 * never depends on a grid cap.  By default the budget is the number of
 * blocks the device holds at once: a launch that fits keeps one sub-tile
 * per block, a larger one grows the span until the grid is a single
 * resident wave (measured best at the bench's 3.5M-row launches: S=2,
 * profiles/tile_update_note.md).  PBLOCKS or a forced block count replace
 * the budget, TILE_S the span itself. */
static int launch_tile(GpuOp *o, const UpdateArgs &A) {
    if (!cols_vec_ok(A)) {
        launch_batch(o, A);
        return 0;
    }
    auto kern = k_update_tile<8, TILE_SLOTS, TILE_PROBES>;
    if (o->bq == 16) kern = k_update_tile<16, TILE_SLOTS, TILE_PROBES>;
    else if (o->bq == 12) kern = k_update_tile<12, TILE_SLOTS, TILE_PROBES>;
    if (!o->tile_resident) {
        int per_cu = 0, cus = 0;
        hipError_t e1 = hipOccupancyMaxActiveBlocksPerMultiprocessor(
            &per_cu, kern, 256, 0);
        hipError_t e2 = hipDeviceGetAttribute(
            &cus, hipDeviceAttributeMultiprocessorCount, o->cfg.device);
        HIP_CHECK(o, e1);
        HIP_CHECK(o, e2);
        o->tile_resident = per_cu * cus > 0 ? per_cu * cus : 1;
    }
    int64_t tiles = (A.n_rows / o->bq + 255) / 256;
    if (tiles < 1) tiles = 1;
    int64_t budget = o->tile_resident;
    if (o->pblocks_set) budget = o->pblocks;
    if (o->force_blocks > 0) budget = o->force_blocks;
    if (budget < 1) budget = 1;
    int64_t span = (tiles + budget - 1) / budget;
    if (o->tile_s > 0) span = o->tile_s;
    int blocks = (int)((tiles + span - 1) / span);
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(256), 0, o->stream, A,
                       (int)span);
    launch_batch_tail(o, A);
    return 0;
}

/* launch the update kernel over device-resident columns */
static int launch_update(GpuOp *o, const int64_t *const *dcols, int64_t n_rows,
                         uint64_t ts_offset) {
    if (n_rows == 0) return 0;
    UpdateArgs A = {};
    int c = 0;
    A.key_col = o->cfg.n_keys ? dcols[c++] : nullptr;
    for (int v = 0; v < o->cfg.n_value_cols; v++) A.vcols[v] = dcols[c++];
    A.ts_col = dcols[c];
    A.n_rows = n_rows;
    A.slide = o->slide;
    A.slide_inv = o->slide == 1
                      ? ~0ULL
                      : (uint64_t)((((unsigned __int128)1) << 64) / o->slide);
    A.has_wm = o->has_wm;
    A.wm_bin = o->has_wm ? o->wm - o->wm % o->slide : 0;
    A.ts_offset = ts_offset;
    A.ring = o->ring;
    A.agg = o->agg;
    /* sample kernel time on a subset of launches via a reusable event pool */
    bool sample = o->use_events && (o->launches & 7) == 0;
    if (sample && o->ev_pool.empty()) {
        o->ev_pool.resize(EV_POOL);
        for (auto &pr : o->ev_pool) {
            HIP_CHECK(o, o->event_create(&pr.first));
            HIP_CHECK(o, o->event_create(&pr.second));
        }
    }
    if (sample && o->ev_inflight.size() >= EV_POOL) harvest_events(o, 1);
    int ev = -1;
    if (sample) {
        /* find a free pair: pool minus inflight (inflight cleared on
         * harvest, so pool scan order is fine) */
        ev = (int)(o->ev_inflight.size());
        hipEventRecord(o->ev_pool[ev].first, o->stream);
    }
    switch (o->upd_kind) {
    case UPD_LDS: launch_lds(o, A); break;
    case UPD_BATCH: launch_batch(o, A); break;
    case UPD_TILE:
        if (launch_tile(o, A)) return 1;
        break;
    }
    if (sample) {
        hipEventRecord(o->ev_pool[ev].second, o->stream);
        o->ev_inflight.push_back(ev);
    }
    HIP_CHECK(o, hipGetLastError());
    o->update_rows += n_rows;
    o->launches++;
    return 0;
}

/* normalize a batch's composite keys to dictionary ids (device cols) */
static int mk_encode(GpuOp *o, const int64_t *const *kcols, int64_t n_rows) {
    if (n_rows > o->keyid_in_cap) {
        o->release(o->d_keyid_in);
        o->keyid_in_cap = 0;
        HIP_CHECK(o, o->dev_alloc(o->d_keyid_in,
                                  (size_t)(n_rows + (n_rows >> 2)) * 8));
        o->keyid_in_cap = n_rows + (n_rows >> 2);
    }
    DictEncArgs E = {};
    for (int k = 0; k < o->cfg.n_keys; k++) E.kcols[k] = kcols[k];
    E.nk = o->cfg.n_keys;
    E.n_rows = n_rows;
    E.digest = o->d_dict_digest;
    E.dkeys = o->d_dict_keys;
    E.ready = o->d_dict_ready;
    E.ids = o->d_keyid_in;
    E.D = o->dict_D;
    E.err = o->ring.err;
    int64_t want = (n_rows + 255) / 256;
    int blocks = (int)(want > 2048 ? 2048 : (want < 1 ? 1 : want));
    hipLaunchKernelGGL(k_dict_encode, dim3(blocks), dim3(256), 0, o->stream,
                       E);
    HIP_CHECK(o, hipGetLastError());
    return 0;
}

/* build the single-key engine view of a user batch: [ids, vals..., ts] */
static int mk_engine_cols(GpuOp *o, const int64_t *const *dcols,
                          int64_t n_rows, const int64_t **eng) {
    if (mk_encode(o, dcols, n_rows)) return 1;
    int c = 0;
    eng[c++] = o->d_keyid_in;
    for (int v = 0; v < o->cfg.n_value_cols; v++)
        eng[c++] = dcols[o->cfg.n_keys + v];
    eng[c] = dcols[o->cfg.n_keys + o->cfg.n_value_cols];
    return 0;
}

static int flush_staged(GpuOp *o) {
    if (o->stg.n == 0) return 0;
    /* up to 4 key + 4 value columns + ts; the engine view below has one key */
    const int64_t *dcols[OP_STG_MAX_COLS];
    if (o->stg.upload(o, o->n_in_cols, o->stg.n, dcols)) return 1;
    int rc;
    if (o->mk) {
        const int64_t *eng[6];
        if (mk_engine_cols(o, dcols, o->stg.n, eng)) return 1;
        rc = launch_update(o, eng, o->stg.n, 0);
    } else {
        rc = launch_update(o, dcols, o->stg.n, 0);
    }
    o->stg.n = 0;
    return rc;
}

API int arroyo_amd_process_batch(void *h, const int64_t *const *cols,
                                 int32_t n_cols, int64_t n_rows) {
    GpuOp *o = (GpuOp *)h;
    if (n_cols != o->n_in_cols) {
        snprintf(o->err_msg, sizeof o->err_msg, "expected %d cols, got %d",
                 o->n_in_cols, n_cols);
        return 1;
    }
    int64_t done = 0;
    while (done < n_rows) {
        int64_t take = n_rows - done;
        if (take > o->stg.cap - o->stg.n) take = o->stg.cap - o->stg.n;
        for (int i = 0; i < n_cols; i++)
            memcpy(o->stg.h[i] + o->stg.n, cols[i] + done, (size_t)take * 8);
        o->stg.n += take;
        done += take;
        if (o->stg.n == o->stg.cap)
            if (flush_staged(o)) return 1;
    }
    return 0;
}

/* bench path: columns already resident in HBM */
API int arroyo_amd_process_batch_device(void *h, const int64_t *const *dcols,
                                        int32_t n_cols, int64_t n_rows,
                                        uint64_t ts_offset) {
    GpuOp *o = (GpuOp *)h;
    if (n_cols != o->n_in_cols) {
        snprintf(o->err_msg, sizeof o->err_msg, "expected %d cols, got %d",
                 o->n_in_cols, n_cols);
        return 1;
    }
    if (flush_staged(o)) return 1;
    if (o->mk) {
        const int64_t *eng[6];
        if (mk_engine_cols(o, dcols, n_rows, eng)) return 1;
        return launch_update(o, eng, n_rows, ts_offset);
    }
    return launch_update(o, dcols, n_rows, ts_offset);
}

/* replay harness path: submit `reps` consecutive device-resident batches in
 * one call (one kernel launch per batch, ts_offset advancing by ts_step),
 * so the per-batch Python/FFI overhead is off the measured path.  batches
 * are laid out back-to-back in dcols: batch k = rows [k*n_rows, (k+1)*n_rows)
 * when contiguous=1, else the same batch is replayed reps times. */
API int arroyo_amd_process_batches_device(void *h,
                                          const int64_t *const *dcols,
                                          int32_t n_cols, int64_t n_rows,
                                          int32_t reps, int32_t contiguous,
                                          uint64_t ts_offset0,
                                          uint64_t ts_step) {
    GpuOp *o = (GpuOp *)h;
    if (n_cols != o->n_in_cols) {
        snprintf(o->err_msg, sizeof o->err_msg, "expected %d cols, got %d",
                 o->n_in_cols, n_cols);
        return 1;
    }
    if (flush_staged(o)) return 1;
    /* contiguous batches sharing one ts_offset are row-independent work on
     * adjacent memory: fuse them into a single launch (same computation,
     * ~15x the rows per launch -- the reference likewise drains its queue
     * into the per-bin execs in bulk) */
    if (contiguous && ts_step == 0) {
        if (o->mk) {
            const int64_t *eng[6];
            if (mk_engine_cols(o, dcols, n_rows * reps, eng)) return 1;
            return launch_update(o, eng, n_rows * reps, ts_offset0);
        }
        return launch_update(o, dcols, n_rows * reps, ts_offset0);
    }
    const int64_t *cols[16];
    for (int k = 0; k < reps; k++) {
        for (int c = 0; c < n_cols; c++)
            cols[c] = dcols[c] + (contiguous ? (int64_t)k * n_rows : 0);
        if (o->mk) {
            const int64_t *eng[6];
            if (mk_engine_cols(o, cols, n_rows, eng)) return 1;
            if (launch_update(o, eng, n_rows,
                              ts_offset0 + (uint64_t)k * ts_step))
                return 1;
            continue;
        }
        if (launch_update(o, cols, n_rows, ts_offset0 + (uint64_t)k * ts_step))
            return 1;
    }
    return 0;
}

/* busy-wait on an event: the interrupt-based hipEventSynchronize costs
 * 10-20 us of wake-up latency per call, on the watermark critical path */
static int wait_event_spin(GpuOp *o, hipEvent_t ev) {
    if (!o->spin) {
        HIP_CHECK(o, hipEventSynchronize(ev));
        return 0;
    }
    hipError_t e;
    while ((e = hipEventQuery(ev)) == hipErrorNotReady) {}
    (void)hipGetLastError();   /* clear the NotReady sticky */
    if (e != hipSuccess) {
        snprintf(o->err_msg, sizeof o->err_msg, "event wait: %s",
                 hipGetErrorString(e));
        return 1;
    }
    return 0;
}

static int decode_status_error(GpuOp *o, const uint64_t *status);

/* one round trip: pulls err + min_bin + pane tags into h_status */
static int check_device_error(GpuOp *o) {
    HIP_CHECK(o, hipMemcpyAsync(o->h_status, o->d_status,
                                (2 + (size_t)o->ring.R) * 8,
                                hipMemcpyDeviceToHost, o->stream));
    HIP_CHECK(o, hipEventRecord(o->ev_sync, o->stream));
    if (wait_event_spin(o, o->ev_sync)) return 1;
    return decode_status_error(o, o->h_status);
}

static int decode_status_error(GpuOp *o, const uint64_t *status) {
    int e = *(const int *)status;
    if (e == ERR_RING_CONFLICT) {
        snprintf(o->err_msg, sizeof o->err_msg,
                 "pane ring conflict: more than ring_panes=%u live bins; "
                 "raise ring_panes", o->ring.R);
        return 1;
    }
    if (e == ERR_TABLE_FULL) {
        snprintf(o->err_msg, sizeof o->err_msg,
                 "pane hash table full (capacity 2^%u); raise log2_capacity",
                 o->cfg.log2_capacity);
        return 1;
    }
    if (e == ERR_MF_OVERFLOW) {
        snprintf(o->err_msg, sizeof o->err_msg,
                 "fused-merge LDS table overflow (pathological key "
                 "clustering); raise log2_capacity");
        return 1;
    }
    if (e == ERR_DICT_FULL) {
        snprintf(o->err_msg, sizeof o->err_msg,
                 "key dictionary full (capacity %u composite keys over the "
                 "operator lifetime); raise log2_capacity", o->dict_D);
        return 1;
    }
    if (e == ERR_DICT_SPIN) {
        snprintf(o->err_msg, sizeof o->err_msg,
                 "key dictionary publish wait exhausted (device anomaly)");
        return 1;
    }
    if (e) {
        snprintf(o->err_msg, sizeof o->err_msg, "device error %d", e);
        return 1;
    }
    return 0;
}

/* refresh host view of open panes from h_status (populated by
 * check_device_error, which every entry path calls first) */
static int sync_open_panes(GpuOp *o) {
    const uint64_t *tags = o->h_status + 2;
    o->open.clear();
    for (uint32_t s = 0; s < o->ring.R; s++) {
        if (tags[s] == EMPTY_TAG) continue;
        /* a retire launched on the fire stream may not be visible in this
         * snapshot yet; its bin can never be re-claimed (late-dropped) */
        if (s < o->retired_bin.size() && tags[s] == o->retired_bin[s])
            continue;
        bool is_closed = false;
        auto it = o->closed.find(tags[s]);
        if (it != o->closed.end() && it->second == s) is_closed = true;
        if (!is_closed) o->open[tags[s]] = s;
    }
    return 0;
}

/* merge + compact + (optionally) copy out one fired window */
static int fire_window(GpuOp *o, const std::vector<uint32_t> &src,
                       uint64_t ws, uint64_t we, int raw_states,
                       uint64_t bin_ts) {
    size_t na = o->agg.n_aggs;
    /* fused hash-aligned path: one kernel, no merge table, no state
     * atomics (see k_merge_fused); legacy merge+compact otherwise */
    if (!raw_states && na <= MF_MAX_AGGS && o->ring.C >= MF_RANGE &&
        src.size() <= 64) {
        /* alternate the period's independent window merges across the two
         * fire streams (read-only over the panes; retires wait on both).
         * mk is excluded: the dictionary-id scratch column is shared. */
        hipStream_t fs = o->fstream;
        int64_t *const *outv = o->d_out;
        int on_f2 = o->own_fstream && !o->mk && (o->fire_alt & 1);
        o->fire_alt++;
        unsigned long long *cur;
        if (on_f2) {
            /* in-stream order already puts this merge after the group's
             * cpi builds (same stream) and the gate */
            fs = o->fstream2;
            outv = o->d_out2;
            if ((o->fire_seq2 & 63) == 0)
                HIP_CHECK(o, hipMemsetAsync(o->d_fire_cur2, 0, 64 * 8, fs));
            cur = o->d_fire_cur2 + (o->fire_seq2 & 63);
            o->fire_seq2++;
        } else {
            /* cpi builds run on fstream2: order this merge after them */
            if (o->own_fstream)
                HIP_CHECK(o, hipStreamWaitEvent(o->fstream, o->ev_cpi, 0));
            if ((o->fire_seq & 63) == 0)
                HIP_CHECK(o, hipMemsetAsync(o->d_fire_cur, 0, 64 * 8, fs));
            cur = o->d_fire_cur + (o->fire_seq & 63);
            o->fire_seq++;
        }
        o->last_cur[on_f2] = cur;
        if (!src.empty()) {
            MergeFusedArgs M = {};
            M.ring = o->ring;
            M.agg = o->agg;
            M.n_src = (int)src.size();
            for (size_t i = 0; i < src.size(); i++) M.src[i] = src[i];
            M.win_start = ws;
            M.win_end = we;
            M.n_keys = o->cfg.n_keys ? 1 : 0;
            if (o->mk) {
                /* engine emits the dictionary id; decode expands it into
                 * the k key columns afterwards */
                M.out[0] = o->d_keyid_out;
                for (int i = 1; i < o->n_out_alloc - o->cfg.n_keys + 1 &&
                                i < 16; i++)
                    M.out[i] = outv[o->cfg.n_keys - 1 + i];
            } else {
                for (int i = 0; i < o->n_out_alloc && i < 16; i++)
                    M.out[i] = outv[i];
            }
            M.n_out = cur;
            /* emitted-row accounting folded into the kernel for the
             * device-resident path (saves the separate k_accum launch) */
            M.accum = o->cfg.emit_to_host ? nullptr : o->d_emitted;
            /* 1024 slots won the round-1 sweep (3->4 workgroups per CU);
             * typical occupancy is ~320 owned keys per 256-slot home range
             * and overflow is a loud error, not silent corruption.  Larger
             * ranges cut the overscan ratio (range+256)/range but need the
             * 2048-slot table. */
            int mfs = 1024;
            if (const char *ev = getenv("ARROYO_AMD_MF_SLOTS"))
                mfs = atoi(ev);
            uint32_t range = o->mf_range;
            M.range = range;
            M.use_cpi = 0;
            if (o->cpi_entries && src.size() <= 16) {
                int all = 1;
                for (size_t i = 0; i < src.size(); i++)
                    if (!o->cpi_ready[src[i]]) all = 0;
                if (all) {
                    M.use_cpi = 1;
                    M.cpi_ew = o->cpi_ew;
                    M.cpi_range = o->cpi_range;
                    for (size_t i = 0; i < src.size(); i++) {
                        M.cpi_entries[i] =
                            o->cpi_entries +
                            (size_t)src[i] * o->ring.C * o->cpi_ew;
                        M.cpi_cnt[i] =
                            o->cpi_cnt + (size_t)src[i] * o->cpi_nr;
                    }
                }
            }
            int slots = mfs >= 4096 ? 4096 : (mfs >= 2048 ? 2048 : 1024);
            if (slots == 4096 && !(M.use_cpi && o->cpi_ew == 2))
                slots = 2048;   /* 4096 two-word states blow the LDS */
            size_t shmem = (size_t)slots *
                           ((M.use_cpi && o->cpi_ew == 2) ? 8 : na * 16);
            if (slots == 4096)
                hipLaunchKernelGGL(k_merge_fused<4096>,
                                   dim3(o->ring.C / range), dim3(256),
                                   shmem, fs, M);
            else if (slots == 2048)
                hipLaunchKernelGGL(k_merge_fused<2048>,
                                   dim3(o->ring.C / range), dim3(256),
                                   shmem, fs, M);
            else
                hipLaunchKernelGGL(k_merge_fused<1024>,
                                   dim3(o->ring.C / range), dim3(256),
                                   shmem, fs, M);
            HIP_CHECK(o, hipGetLastError());
            if (o->mk) {
                DictDecArgs DD = {};
                DD.ids = o->d_keyid_out;
                DD.n = cur;
                DD.dkeys = o->d_dict_keys;
                DD.nk = o->cfg.n_keys;
                for (int k = 0; k < o->cfg.n_keys; k++) DD.out[k] = outv[k];
                hipLaunchKernelGGL(k_dict_decode, dim3(1024), dim3(256), 0,
                                   fs, DD);
                HIP_CHECK(o, hipGetLastError());
            }
        }
        if (!o->cfg.emit_to_host) {
            if (on_f2) {
                HIP_CHECK(o, hipEventRecord(o->ev_f2, o->fstream2));
                o->f2_dirty = 1;
            }
            return 0;
        }
        unsigned long long n = 0;
        HIP_CHECK(o, hipMemcpyAsync(&n, cur, 8,
                                    hipMemcpyDeviceToHost, fs));
        HIP_CHECK(o, hipStreamSynchronize(fs));
        if (n == 0) return 0;
        if ((size_t)o->out_cols > o->host_out.size())
            o->host_out.resize(o->out_cols);
        for (int i = 0; i < o->out_cols; i++) {
            size_t old = o->host_out[i].size();
            o->host_out[i].resize(old + n);
            HIP_CHECK(o, hipMemcpyAsync(o->host_out[i].data() + old,
                                        outv[i], n * 8,
                                        hipMemcpyDeviceToHost, fs));
        }
        HIP_CHECK(o, hipStreamSynchronize(fs));
        return 0;
    }
    HIP_CHECK(o, hipMemsetAsync(o->m_keys, 0xFF, (size_t)o->CM * 8, o->stream));
    HIP_CHECK(o, hipMemsetAsync(o->m_zero_blob, 0, o->m_zero_bytes,
                                o->stream));
    if (!src.empty()) {
        MergeArgs M = {};
        M.ring = o->ring;
        M.agg = o->agg;
        M.m_keys = o->m_keys;
        M.m_state = o->m_state;
        M.m_spec_used = o->m_spec_used;
        M.m_spec_state = o->m_spec_state;
        M.CM = o->CM;
        M.n_src = (int)src.size();
        for (size_t i = 0; i < src.size() && i < 64; i++) M.src[i] = src[i];
        size_t total = (size_t)M.n_src * o->ring.C;
        int blocks = (int)((total + 255) / 256);
        if (blocks > 4096) blocks = 4096;
        hipLaunchKernelGGL(k_merge, dim3(blocks), dim3(256), 0, o->stream, M);
        HIP_CHECK(o, hipGetLastError());
    }
    CompactArgs C = {};
    C.m_keys = o->m_keys;
    C.m_state = o->m_state;
    C.m_spec_used = o->m_spec_used;
    C.m_spec_state = o->m_spec_state;
    C.CM = o->CM;
    C.agg = o->agg;
    C.n_keys = o->cfg.n_keys ? 1 : 0;
    C.raw_states = raw_states;
    C.win_start = raw_states ? bin_ts : ws;
    C.win_end = we;
    if (o->mk) {
        C.out[0] = o->d_keyid_out;
        for (int i = 1; i < o->n_out_alloc - o->cfg.n_keys + 1 && i < 16; i++)
            C.out[i] = o->d_out[o->cfg.n_keys - 1 + i];
    } else {
        for (int i = 0; i < o->n_out_alloc && i < 16; i++)
            C.out[i] = o->d_out[i];
    }
    C.n_out = o->d_n_out;
    /* a raw-state drain overwrites d_out: no window emission left there */
    o->last_cur[0] = raw_states ? nullptr : o->d_n_out;
    int blocks = (int)((o->CM + 255) / 256);
    if (blocks > 1024) blocks = 1024;   /* 1 global cursor atomic per block */
    hipLaunchKernelGGL(k_compact, dim3(blocks), dim3(256), 0, o->stream, C);
    HIP_CHECK(o, hipGetLastError());
    if (o->mk) {
        DictDecArgs DD = {};
        DD.ids = o->d_keyid_out;
        DD.n = o->d_n_out;
        DD.dkeys = o->d_dict_keys;
        DD.nk = o->cfg.n_keys;
        for (int k = 0; k < o->cfg.n_keys; k++) DD.out[k] = o->d_out[k];
        hipLaunchKernelGGL(k_dict_decode, dim3(1024), dim3(256), 0,
                           o->stream, DD);
        HIP_CHECK(o, hipGetLastError());
    }
    if (!o->cfg.emit_to_host && !raw_states) {
        /* device-resident emission: the next pipeline stage's collector
         * consumes d_out in place.  Accounting stays on device so firing
         * costs NO host round trip; perf() folds the accumulator in. */
        hipLaunchKernelGGL(k_accum, dim3(1), dim3(1), 0, o->stream,
                           o->d_emitted, o->d_n_out);
        HIP_CHECK(o, hipGetLastError());
        /* legacy merges run on the main stream but share d_out/d_n_out
         * and panes with fire-stream work: re-gate so later fire-stream
         * launches order after them */
        return gate_fire(o);
    }
    unsigned long long n = 0;
    HIP_CHECK(o, hipMemcpyAsync(&n, o->d_n_out, 8, hipMemcpyDeviceToHost,
                                o->stream));
    HIP_CHECK(o, hipStreamSynchronize(o->stream));
    if (n == 0) return gate_fire(o);
    int ncols = raw_states ? 0 : o->out_cols;
    if (raw_states) {
        ncols = o->cfg.n_keys + 1;
        for (int a = 0; a < o->agg.n_aggs; a++)
            ncols += (o->agg.op[a] == AMD_AGG_AVG) ? 2 : 1;
    }
    if (o->cfg.emit_to_host || raw_states) {
        if ((size_t)ncols > o->host_out.size()) o->host_out.resize(ncols);
        for (int i = 0; i < ncols; i++) {
            size_t old = o->host_out[i].size();
            o->host_out[i].resize(old + n);
            HIP_CHECK(o, hipMemcpyAsync(o->host_out[i].data() + old,
                                        o->d_out[i], n * 8,
                                        hipMemcpyDeviceToHost, o->stream));
        }
        HIP_CHECK(o, hipStreamSynchronize(o->stream));
    }
    return gate_fire(o);
}

/* pair launch: one k_merge_dual over the union of two consecutive
 * windows' panes (COUNT shape; see the kernel) */
static int fire_dual(GpuOp *o, const GpuOp::PendFire &A,
                     const GpuOp::PendFire &B) {
    hipStream_t fs = o->fstream;
    if (o->own_fstream)
        HIP_CHECK(o, hipStreamWaitEvent(o->fstream, o->ev_cpi, 0));
    if ((o->fire_seq & 63) == 0)
        HIP_CHECK(o, hipMemsetAsync(o->d_fire_cur, 0, 64 * 8, fs));
    unsigned long long *cur = o->d_fire_cur + (o->fire_seq & 63);
    o->fire_seq++;
    o->fire_alt++;
    o->last_cur[0] = cur;
    MergeDualArgs M = {};
    M.ring = o->ring;
    std::vector<uint32_t> uni = A.src;
    for (uint32_t sv : B.src)
        if (std::find(uni.begin(), uni.end(), sv) == uni.end())
            uni.push_back(sv);
    M.n_src = (int)uni.size();
    for (size_t i = 0; i < uni.size(); i++) {
        M.src[i] = uni[i];
        if (std::find(A.src.begin(), A.src.end(), uni[i]) != A.src.end())
            M.maskA |= 1ULL << i;
        if (std::find(B.src.begin(), B.src.end(), uni[i]) != B.src.end())
            M.maskB |= 1ULL << i;
        M.cpi_entries[i] = o->cpi_entries +
                           (size_t)uni[i] * o->ring.C * o->cpi_ew;
        M.cpi_cnt[i] = o->cpi_cnt + (size_t)uni[i] * o->cpi_nr;
    }
    M.wsA = A.ws;
    M.weA = A.we;
    M.wsB = B.ws;
    M.weB = B.we;
    M.n_keys = o->cfg.n_keys ? 1 : 0;
    M.range = o->mf_range;
    M.cpi_range = o->cpi_range;
    for (int i = 0; i < o->n_out_alloc && i < 8; i++) M.out[i] = o->d_out[i];
    M.n_out = cur;
    M.accum = o->cfg.emit_to_host ? nullptr : o->d_emitted;
    size_t shmem = (size_t)2048 * 2 * 8;
    hipLaunchKernelGGL(k_merge_dual<2048>, dim3(o->ring.C / o->mf_range),
                       dim3(256), shmem, fs, M);
    HIP_CHECK(o, hipGetLastError());
    if (!o->cfg.emit_to_host) return 0;
    unsigned long long n = 0;
    HIP_CHECK(o, hipMemcpyAsync(&n, cur, 8, hipMemcpyDeviceToHost, fs));
    HIP_CHECK(o, hipStreamSynchronize(fs));
    if (n == 0) return 0;
    if ((size_t)o->out_cols > o->host_out.size())
        o->host_out.resize(o->out_cols);
    for (int i = 0; i < o->out_cols; i++) {
        size_t old = o->host_out[i].size();
        o->host_out[i].resize(old + n);
        HIP_CHECK(o, hipMemcpyAsync(o->host_out[i].data() + old,
                                    o->d_out[i], n * 8,
                                    hipMemcpyDeviceToHost, fs));
    }
    HIP_CHECK(o, hipStreamSynchronize(fs));
    return 0;
}

/* can this op use k_merge_dual at all? */
static int dual_ok(GpuOp *o) {
    /* default OFF: at the bench balance the union table's higher LDS
     * load factor and doubled shared-pane atomics cost ~1.2% more than
     * the 10->6 pane-read saving buys (same-box A/B x2); the trade may
     * flip for wider windows (width/slide > 5) where the sharing grows.
     * Read per call (not latched) so tests can exercise the path. */
    const char *ev = getenv("ARROYO_AMD_DUAL");
    int on = ev ? atoi(ev) != 0 : 0;
    return on && o->cpi_entries && o->cpi_ew == 2 && !o->mk &&
           o->agg.n_aggs == 1 && o->agg.op[0] == AMD_AGG_COUNT &&
           !o->agg.isf[0];
}

/* fire (or queue, when a batched call may pair it) one window */
static int queue_fire(GpuOp *o, const std::vector<uint32_t> &src,
                      uint64_t ws, uint64_t we) {
    if (!o->defer_fires)
        return fire_window(o, src, ws, we, 0, 0);
    o->pend_fires.push_back({src, ws, we});
    return 0;
}

static int queue_retire(GpuOp *o, uint32_t slot, uint64_t bin) {
    if (!o->defer_fires) return ring_retire(o, slot, bin);
    o->pend_retires.push_back({slot, bin});
    return 0;
}

/* launch queued fires (pairing consecutive windows whose panes all have
 * a closed-pane index) then the queued retires */
static int flush_pend(GpuOp *o) {
    size_t i = 0;
    while (i < o->pend_fires.size()) {
        GpuOp::PendFire &a = o->pend_fires[i];
        int paired = 0;
        if (i + 1 < o->pend_fires.size()) {
            GpuOp::PendFire &b = o->pend_fires[i + 1];
            int ready = a.src.size() + b.src.size() <= 16 &&
                        !a.src.empty() && !b.src.empty() &&
                        b.ws == a.ws + o->slide && b.we == a.we + o->slide;
            if (ready)
                for (uint32_t sv : a.src)
                    if (!(sv < o->cpi_ready.size() && o->cpi_ready[sv]))
                        ready = 0;
            if (ready)
                for (uint32_t sv : b.src)
                    if (!(sv < o->cpi_ready.size() && o->cpi_ready[sv]))
                        ready = 0;
            if (ready) {
                if (fire_dual(o, a, b)) return 1;
                i += 2;
                paired = 1;
            }
        }
        if (!paired) {
            if (fire_window(o, a.src, a.ws, a.we, 0, 0)) return 1;
            i += 1;
        }
    }
    o->pend_fires.clear();
    for (auto &pr : o->pend_retires)
        if (ring_retire_planes(o, pr.first, pr.second)) return 1;
    o->pend_retires.clear();
    return ring_retire_flush(o);
}

/* advance(): sliding_aggregating_window.rs:115-210, host replica */
static int advance(GpuOp *o) {
    uint64_t b = (o->state == 1) ? o->earliest : o->next_start;
    uint64_t E = b + o->slide;

    /* flush retention cutoff (retention = width) */
    if (E >= o->width) {
        uint64_t cut = E - o->width;
        for (auto it = o->table_bins.begin();
             it != o->table_bins.end() && *it < cut;)
            it = o->table_bins.erase(it);
    }
    auto op_it = o->open.find(b);
    if (op_it != o->open.end()) {
        o->closed[b] = op_it->second;   /* pane stays in the ring */
        if (cpi_build(o, op_it->second)) return 1;
        o->open.erase(op_it);
        o->table_bins.insert(b);
    }
    if (E + o->slide >= o->width)
        o->table_bins.erase(E + o->slide - o->width);

    std::vector<uint32_t> src;
    uint64_t lo = (E >= o->width) ? E - o->width : 0;
    for (auto &kv : o->closed)
        if (kv.first >= lo && kv.first < E) src.push_back(kv.second);

    /* delete_before(E + slide - width): retire ring slots */
    uint64_t del = (E + o->slide >= o->width) ? E + o->slide - o->width : 0;
    std::vector<uint64_t> dead;
    for (auto &kv : o->closed)
        if (kv.first < del) dead.push_back(kv.first);

    if (queue_fire(o, src, E - o->width, E)) return 1;

    for (uint64_t bb : dead) {
        if (queue_retire(o, o->closed[bb], bb)) return 1;
        o->closed.erase(bb);
    }
    if (!o->defer_fires && ring_retire_flush(o)) return 1;

    if (o->closed.empty()) {
        if (!o->table_bins.empty()) {
            o->state = 1;
            uint64_t m = *o->table_bins.begin();
            o->earliest = m - m % o->slide;
        } else {
            o->state = 0;
        }
    } else {
        o->state = 2;
        o->next_start = E;
    }
    return 0;
}

static int build_out(GpuOp *o, AmdOutBatch *out, int raw_states) {
    int ncols = o->out_cols;
    if (raw_states) {
        ncols = o->cfg.n_keys + 1;
        for (int a = 0; a < o->agg.n_aggs; a++)
            ncols += (o->agg.op[a] == AMD_AGG_AVG) ? 2 : 1;
    }
    int64_t n = o->host_out.empty() ? 0 : (int64_t)o->host_out[0].size();
    /* loud error per the library convention, never a null-deref */
    if (op_out_alloc(o, out, n, ncols, "build_out")) return 1;
    for (int i = 0; n && i < ncols; i++)
        memcpy(out->cols[i], o->host_out[i].data(), (size_t)n * 8);
    if (!raw_states) {
        for (int a = 0; a < o->agg.n_aggs; a++)
            if (o->agg.op[a] == AMD_AGG_AVG || o->agg.isf[a])
                out->is_f64[o->cfg.n_keys + a] = 1;
    } else {
        int col = o->cfg.n_keys;
        for (int a = 0; a < o->agg.n_aggs; a++) {
            if (o->agg.op[a] == AMD_AGG_AVG) {
                out->is_f64[col + 1] = 1;
                col += 2;
            } else {
                if (o->agg.isf[a]) out->is_f64[col] = 1;
                col += 1;
            }
        }
    }
    for (auto &v : o->host_out) v.clear();
    return 0;
}

/* per-watermark firing logic, after the (shared) device status fold */
static int wm_advance(GpuOp *o, uint64_t wm) {
    o->has_wm = 1;
    o->wm = wm;
    uint64_t wb = wm - wm % o->slide;

    if (o->cfg.is_tumbling) {
        /* tumbling_aggregating_window.rs:321-392 */
        while (!o->open.empty() && o->open.begin()->first < wb) {
            uint64_t b = o->open.begin()->first;
            uint32_t slot = o->open.begin()->second;
            std::vector<uint32_t> src = {slot};
            if (fire_window(o, src, b, b + o->width, 0, 0)) return 1;
            if (ring_retire_planes(o, slot, b)) return 1;
            o->open.erase(o->open.begin());
        }
        if (ring_retire_flush(o)) return 1;
    } else {
        while (o->state != 0) {
            uint64_t base = (o->state == 1) ? o->earliest : o->next_start;
            if (!(base + o->slide <= wb)) break;
            if (advance(o)) return 1;
        }
        /* unreachable open panes (the reference leaks these silently --
         * sliding state machine NoData/jump quirk): retire so the ring
         * slot is reusable; their rows are dropped either way */
        uint64_t base = (o->state == 1)   ? o->earliest
                        : (o->state == 2) ? o->next_start
                                          : ~0ULL;
        std::vector<uint64_t> unreachable;
        for (auto &kv : o->open)
            if (kv.first + o->slide <= wb && kv.first < base)
                unreachable.push_back(kv.first);
        for (uint64_t bb : unreachable) {
            if (ring_retire_planes(o, o->open[bb], bb)) return 1;
            o->open.erase(bb);
        }
        if (ring_retire_flush(o)) return 1;
    }
    return 0;
}

/* fold the device status (error, min non-late bin, pane tags) into the
 * host state machine: ONE copy + sync */
static int wm_fold_status(GpuOp *o) {
    if (flush_staged(o)) return 1;
    if (check_device_error(o)) return 1;
    harvest_events(o, 0);
    if (sync_open_panes(o)) return 1;
    /* the OnlyBufferedData `earliest` only advances while not
     * InMemoryData; arrivals during InMemoryData are intentionally not
     * folded -- see sliding_aggregating_window.rs:635-647 */
    uint64_t minb = o->h_status[1];
    HIP_CHECK(o, hipMemsetAsync(o->ring.min_bin, 0xFF, 8, o->stream));
    if (!o->cfg.is_tumbling && minb != ~0ULL) {
        if (o->state == 0) {
            o->state = 1;
            o->earliest = minb;
        } else if (o->state == 1 && minb < o->earliest) {
            o->earliest = minb;
        }
    }
    /* the lag wait goes AFTER the blocking status sync above: it only
     * has to precede the NEXT groups' update launches -- enqueued before
     * the copy it would stall the host on the whole previous fire group
     * (measured -25% whole-job) */
    if (bound_fire_lag(o)) return 1;
    return gate_fire(o);
}

API int arroyo_amd_handle_watermark(void *h, uint64_t wm, AmdOutBatch *out) {
    GpuOp *o = (GpuOp *)h;
    if (wm_fold_status(o)) return 1;
    o->defer_fires = dual_ok(o);
    int rc = wm_advance(o, wm);
    if (!rc) rc = flush_pend(o);
    o->defer_fires = 0;
    if (rc) {
        o->pend_fires.clear();   /* a failed group must not leak deferred
                                    work into the next call */
        o->pend_retires.clear();
        return 1;
    }
    if (fire_tail(o)) return 1;
    if (out) return build_out(o, out, 0);
    return 0;
}

/* batched watermarks with NO rows between them (the harness's fused
 * watermark periods): the pane tags and min-bin cannot change between
 * the emissions, so one status round trip serves every watermark --
 * the per-watermark copy+sync was ~15 us of stream idle each */
API int arroyo_amd_handle_watermarks(void *h, const uint64_t *wms,
                                     int32_t n, AmdOutBatch *out) {
    GpuOp *o = (GpuOp *)h;
    if (n <= 0) return 0;
    if (wm_fold_status(o)) return 1;
    o->defer_fires = dual_ok(o);
    int rc = 0;
    for (int32_t i = 0; i < n && !rc; i++) rc = wm_advance(o, wms[i]);
    if (!rc) rc = flush_pend(o);
    o->defer_fires = 0;
    if (rc) {
        o->pend_fires.clear();
        o->pend_retires.clear();
        return 1;
    }
    if (fire_tail(o)) return 1;
    if (out) return build_out(o, out, 0);
    return 0;
}

/* ---- epoch pipelining -------------------------------------------------
 * The sequential order is submit(g) -> fold+fire(g) -> submit(g+1): the
 * host blocks in the fold until period g's update kernels finish, leaving
 * the main stream idle.  mark_epoch snapshots the device status (pane
 * tags + min non-late bin) on the stream right after period g's launches,
 * so the harness may submit period g+1 BEFORE folding g's watermarks:
 *
 *   submit(g); mark_epoch(); set_filter_watermark(last wm of g);
 *   submit(g+1); handle_watermarks_epoch(g's wms);
 *
 * set_filter_watermark pre-advances the ingest late-drop cutoff to the
 * value the deferred watermarks will establish, so period g+1's rows are
 * filtered EXACTLY as in the sequential order (without it, a row late
 * under g's watermark could land in a pane g's fires read concurrently).
 * Depth 2; emissions and state are bit-identical to the sequential calls
 * (tests/test_gpu_parity.py::test_epoch_pipelined_equals_sequential). */

API int arroyo_amd_set_filter_watermark(void *h, uint64_t wm) {
    GpuOp *o = (GpuOp *)h;
    o->has_wm = 1;
    o->wm = wm;
    return 0;
}

API int arroyo_amd_mark_epoch(void *h) {
    GpuOp *o = (GpuOp *)h;
    if (o->epoch_cnt >= 2) {
        snprintf(o->err_msg, sizeof o->err_msg,
                 "epoch queue full (depth 2): fold the oldest epoch with "
                 "handle_watermarks_epoch first");
        return 1;
    }
    if (flush_staged(o)) return 1;
    int e = (o->epoch_head + o->epoch_cnt) & 1;
    HIP_CHECK(o, hipMemcpyAsync(o->h_epoch[e], o->d_status,
                                (2 + (size_t)o->ring.R) * 8,
                                hipMemcpyDeviceToHost, o->stream));
    /* reset AFTER the snapshot captured it (stream order) */
    HIP_CHECK(o, hipMemsetAsync(o->ring.min_bin, 0xFF, 8, o->stream));
    HIP_CHECK(o, hipEventRecord(o->ev_epoch[e], o->stream));
    o->epoch_cnt++;
    return 0;
}

API int arroyo_amd_handle_watermarks_epoch(void *h, const uint64_t *wms,
                                           int32_t n, AmdOutBatch *out) {
    GpuOp *o = (GpuOp *)h;
    if (o->epoch_cnt == 0) {
        snprintf(o->err_msg, sizeof o->err_msg,
                 "no armed epoch: call mark_epoch after the period's rows");
        return 1;
    }
    int e = o->epoch_head;
    o->epoch_head ^= 1;
    o->epoch_cnt--;
    if (wait_event_spin(o, o->ev_epoch[e])) return 1;
    if (decode_status_error(o, o->h_epoch[e])) return 1;
    harvest_events(o, 0);
    /* fold from the epoch's snapshot */
    memcpy(o->h_status, o->h_epoch[e], (2 + (size_t)o->ring.R) * 8);
    if (sync_open_panes(o)) return 1;
    uint64_t minb = o->h_status[1];
    if (!o->cfg.is_tumbling && minb != ~0ULL) {
        if (o->state == 0) {
            o->state = 1;
            o->earliest = minb;
        } else if (o->state == 1 && minb < o->earliest) {
            o->earliest = minb;
        }
    }
    if (bound_fire_lag(o)) return 1;
    /* gate this epoch's fires on ITS stream point (later periods' update
     * launches are after it and not waited on) */
    if (o->fstream != o->stream) {
        HIP_CHECK(o, hipStreamWaitEvent(o->fstream, o->ev_epoch[e], 0));
        HIP_CHECK(o, hipStreamWaitEvent(o->fstream2, o->ev_epoch[e], 0));
    }
    o->defer_fires = dual_ok(o);
    int rc = 0;
    for (int32_t i = 0; i < n && !rc; i++) rc = wm_advance(o, wms[i]);
    if (!rc) rc = flush_pend(o);
    o->defer_fires = 0;
    if (rc) {
        o->pend_fires.clear();
        o->pend_retires.clear();
        return 1;
    }
    if (fire_tail(o)) return 1;
    if (out) return build_out(o, out, 0);
    return 0;
}

API int arroyo_amd_checkpoint_drain(void *h, AmdOutBatch *out) {
    /* handle_checkpoint (sliding:693-737): open bins' partial states are
     * drained into the state table; raw partial-state layout with the bin
     * as trailing timestamp column. */
    GpuOp *o = (GpuOp *)h;
    HIP_CHECK(o, hipStreamSynchronize(o->fstream));
    if (o->fstream != o->stream)
        HIP_CHECK(o, hipStreamSynchronize(o->fstream2));
    if (flush_staged(o)) return 1;
    if (check_device_error(o)) return 1;
    if (sync_open_panes(o)) return 1;
    for (auto &v : o->host_out) v.clear();
    for (auto &kv : o->open) {
        std::vector<uint32_t> src = {kv.second};
        if (fire_window(o, src, kv.first, 0, 1, kv.first)) return 1;
        o->table_bins.insert(kv.first);
    }
    return build_out(o, out, 1);
}

API int arroyo_amd_restore(void *h, const int64_t *const *cols,
                           int32_t n_cols, int64_t n_rows, int has_wm,
                           uint64_t wm) {
    /* on_start (sliding:556-595): state rows with bin < watermark bin go to
     * the tiered holder (closed panes); others re-open their pane. */
    GpuOp *o = (GpuOp *)h;
    HIP_CHECK(o, hipStreamSynchronize(o->fstream));
    o->retired_bin.assign(o->ring.R, EMPTY_TAG);
    int swords_total = 0;
    int32_t swords[AMD_MAX_AGGS];
    for (int a = 0; a < o->agg.n_aggs; a++) {
        swords[a] = (o->agg.op[a] == AMD_AGG_AVG) ? 2 : 1;
        swords_total += swords[a];
    }
    int want = o->cfg.n_keys + swords_total + 1;
    if (n_cols != want) {
        snprintf(o->err_msg, sizeof o->err_msg,
                 "restore expects %d cols, got %d", want, n_cols);
        return 1;
    }
    uint64_t wmb = has_wm ? wm - wm % o->slide : 0;
    const int64_t *ts = cols[n_cols - 1];
    /* group rows by bin on host, then insert per pane */
    std::map<uint64_t, std::vector<int64_t>> by_bin;
    for (int64_t r = 0; r < n_rows; r++)
        by_bin[(uint64_t)ts[r] - (uint64_t)ts[r] % o->slide].push_back(r);
    for (auto &kv : by_bin) {
        uint64_t bin = kv.first;
        uint32_t p = (uint32_t)((bin / o->slide) & (o->ring.R - 1));
        /* claim ring slot on host: upload tag */
        uint64_t cur;
        HIP_CHECK(o, hipMemcpy(&cur, o->ring.tag + p, 8,
                               hipMemcpyDeviceToHost));
        if (cur != EMPTY_TAG && cur != bin) {
            snprintf(o->err_msg, sizeof o->err_msg, "restore ring conflict");
            return 1;
        }
        HIP_CHECK(o, hipMemcpy(o->ring.tag + p, &bin, 8,
                               hipMemcpyHostToDevice));
        /* gather this bin's rows into staging and launch k_restore */
        int64_t n = (int64_t)kv.second.size();
        if (n > o->stg.cap) {
            snprintf(o->err_msg, sizeof o->err_msg,
                     "restore batch too large for staging (%lld)",
                     (long long)n);
            return 1;
        }
        int sc = 0;
        for (int c = 0; c < n_cols - 1; c++) {
            for (int64_t i = 0; i < n; i++)
                o->stg.h[sc][i] = cols[c][kv.second[i]];
            HIP_CHECK(o, hipMemcpyAsync(o->stg.d[sc], o->stg.h[sc],
                                        (size_t)n * 8, hipMemcpyHostToDevice,
                                        o->stream));
            sc++;
        }
        RestoreArgs R = {};
        int c2 = 0;
        if (o->mk) {
            if (mk_encode(o, (const int64_t *const *)o->stg.d, n))
                return 1;
            R.key_col = o->d_keyid_in;
            c2 = o->cfg.n_keys;
        } else {
            R.key_col = o->cfg.n_keys ? o->stg.d[c2++] : nullptr;
        }
        for (int s = 0; s < swords_total; s++) R.scols[s] = o->stg.d[c2++];
        memcpy(R.swords, swords, sizeof swords);
        R.n_rows = n;
        R.pane = p;
        R.ring = o->ring;
        R.agg = o->agg;
        int blocks = (int)((n + 255) / 256);
        if (blocks > 4096) blocks = 4096;
        hipLaunchKernelGGL(k_restore, dim3(blocks), dim3(256), 0, o->stream, R);
        HIP_CHECK(o, hipGetLastError());
        HIP_CHECK(o, hipStreamSynchronize(o->stream));
        o->table_bins.insert(bin);
        if (has_wm && bin < wmb) {
            o->closed[bin] = p;
            if (cpi_build(o, p)) return 1;
        } else {
            o->open[bin] = p;
        }
    }
    /* state machine init (sliding:580-593) */
    if (!o->cfg.is_tumbling) {
        if (!o->closed.empty()) {
            o->state = 2;
            o->next_start = wmb;
        } else if (!o->table_bins.empty()) {
            o->state = 1;
            uint64_t m = *o->table_bins.begin();
            o->earliest = m - m % o->slide;
        } else {
            o->state = 0;
        }
    }
    if (has_wm) {
        o->has_wm = 1;
        o->wm = wm;
    }
    return 0;
}

API void arroyo_amd_free_out(AmdOutBatch *out) {
    if (!out) return;
    if (out->on_device)   /* device-resident emission (ABI doc) */
        for (int i = 0; out->cols && i < out->n_cols; i++) {
            (void)hipFree(out->cols[i]);
            out->cols[i] = nullptr;
        }
    out_free_host(out);
}

API void arroyo_amd_destroy(void *h) {
    GpuOp *o = (GpuOp *)h;
    if (!o) return;
    harvest_events(o, 1);   /* waits for every sampled launch */
    delete o;
}

/* synchronize the operator's internal stream: callers that reuse receive
 * buffers (the N>1 bench overwrites its RCCL exchange buffers each step)
 * must fence the consuming kernels first */
API int arroyo_amd_sync(void *h) {
    GpuOp *o = (GpuOp *)h;
    HIP_CHECK(o, hipStreamSynchronize(o->stream));
    if (o->fstream != o->stream) {
        HIP_CHECK(o, hipStreamSynchronize(o->fstream));
        HIP_CHECK(o, hipStreamSynchronize(o->fstream2));
    }
    return 0;
}

/* perf introspection for bench.py's roofline leg */
API int arroyo_amd_perf(void *h, double *update_ms, int64_t *rows,
                        int64_t *launches, int64_t *emitted_device_rows) {
    GpuOp *o = (GpuOp *)h;
    harvest_events(o, 1);
    /* update_ms is extrapolated from the sampled launches so that
     * update_ms / launches equals the sampled per-launch average */
    *update_ms = o->sampled_launches
                     ? o->update_kernel_ms *
                           ((double)o->launches / (double)o->sampled_launches)
                     : 0.0;
    *rows = o->update_rows;
    *launches = o->launches;
    /* fold in the device-side fire accumulator (no per-fire round trips) */
    unsigned long long dev_emitted = 0;
    HIP_CHECK(o, hipMemcpyAsync(&dev_emitted, o->d_emitted, 8,
                                hipMemcpyDeviceToHost, o->fstream));
    HIP_CHECK(o, hipStreamSynchronize(o->fstream));
    HIP_CHECK(o, hipMemsetAsync(o->d_emitted, 0, 8, o->fstream));
    *emitted_device_rows = o->emitted_device_rows + (int64_t)dev_emitted;
    o->update_kernel_ms = 0;
    o->sampled_launches = 0;
    o->update_rows = 0;
    o->launches = 0;
    o->emitted_device_rows = 0;
    return 0;
}

/* output introspection for bench.py's --dump-outputs: host copy of the
 * window emissions still resident in the device output buffers -- the
 * latest fire into d_out and, with two fire streams, into d_out2.  Read
 * only; the device-resident path itself never copies these out. */
API int arroyo_amd_last_emission(void *h, AmdOutBatch *out) {
    GpuOp *o = (GpuOp *)h;
    if (arroyo_amd_sync(h)) return 1;
    std::vector<std::vector<int64_t>> rows(o->out_cols);
    for (int b = 0; b < 2; b++) {
        if (!o->last_cur[b]) continue;
        int64_t *const *outv = b ? o->d_out2 : o->d_out;
        unsigned long long n = 0;
        HIP_CHECK(o, hipMemcpy(&n, o->last_cur[b], 8, hipMemcpyDeviceToHost));
        if ((int64_t)n > o->out_rows_cap) {
            snprintf(o->err_msg, sizeof o->err_msg,
                     "last_emission: row cursor %llu exceeds the output "
                     "buffer (%lld rows)", n, (long long)o->out_rows_cap);
            return 1;
        }
        if (n == 0) continue;
        for (int i = 0; i < o->out_cols; i++) {
            size_t old = rows[i].size();
            rows[i].resize(old + n);
            HIP_CHECK(o, hipMemcpy(rows[i].data() + old, outv[i], n * 8,
                                   hipMemcpyDeviceToHost));
        }
    }
    /* build_out packs (and clears) host_out: lend it these rows */
    rows.swap(o->host_out);
    int rc = build_out(o, out, 0);
    rows.swap(o->host_out);
    return rc;
}

/* streaming-read bandwidth calibration (debug/measurement only) */
API double arroyo_amd_stream_gbps(const void *d_a, const void *d_b, int64_t n,
                                  int iters) {
    unsigned long long *d_out;
    if (hipMalloc((void **)&d_out, 8) != hipSuccess) return -1;
    hipMemset(d_out, 0, 8);
    int64_t n2 = n / 2;
    int64_t want = (n2 + 255) / 256;
    int blocks = (int)(want > 8192 ? 8192 : want);
    hipEvent_t t0, t1;
    hipEventCreate(&t0);
    hipEventCreate(&t1);
    hipLaunchKernelGGL(k_stream_sum, dim3(blocks), dim3(256), 0, 0,
                       (const ulonglong2 *)d_a, (const ulonglong2 *)d_b, n2,
                       d_out);
    hipEventRecord(t0, 0);
    for (int i = 0; i < iters; i++)
        hipLaunchKernelGGL(k_stream_sum, dim3(blocks), dim3(256), 0, 0,
                           (const ulonglong2 *)d_a, (const ulonglong2 *)d_b,
                           n2, d_out);
    hipEventRecord(t1, 0);
    hipEventSynchronize(t1);
    float ms = 0;
    hipEventElapsedTime(&ms, t0, t1);
    hipEventDestroy(t0);
    hipEventDestroy(t1);
    hipFree(d_out);
    return (double)n * 16.0 * iters / (ms * 1e-3) / 1e9;
}

/* K8 standalone: partition device-resident rows by key hash for the RCCL
 * all-to-all shuffle (context.rs:506-560 + server_for_hash).  in/out are
 * device pointers; counts is a host pointer receiving per-partition counts. */
API int arroyo_amd_partition(const int64_t *d_keys, const int64_t *d_vals,
                             const int64_t *d_ts, int64_t n, uint32_t n_parts,
                             int64_t *d_out_keys, int64_t *d_out_vals,
                             int64_t *d_out_ts, uint64_t *h_counts) {
    if (n_parts == 0 || n_parts > 64) return 1;
    uint32_t *d_pid;
    unsigned long long *d_counts;
    if (hipMalloc((void **)&d_pid, (size_t)n * 4) != hipSuccess) return 1;
    if (hipMalloc((void **)&d_counts, (size_t)n_parts * 8) != hipSuccess) {
        hipFree(d_pid);
        return 1;
    }
    hipMemset(d_counts, 0, (size_t)n_parts * 8);
    int blocks = (int)((n + 255) / 256);
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(k_partition, dim3(blocks), dim3(256), 0, 0, d_keys, n,
                       n_parts, d_pid, d_counts);
    std::vector<unsigned long long> counts(n_parts);
    hipMemcpy(counts.data(), d_counts, (size_t)n_parts * 8,
              hipMemcpyDeviceToHost);
    std::vector<unsigned long long> cursors(n_parts);
    unsigned long long acc = 0;
    for (uint32_t p = 0; p < n_parts; p++) {
        cursors[p] = acc;
        acc += counts[p];
        h_counts[p] = counts[p];
    }
    hipMemcpy(d_counts, cursors.data(), (size_t)n_parts * 8,
              hipMemcpyHostToDevice);
    hipLaunchKernelGGL(k_scatter, dim3(blocks), dim3(256), 0, 0, d_pid,
                       d_counts, d_keys, d_vals, d_ts, d_out_keys, d_out_vals,
                       d_out_ts, n);
    hipError_t e = hipDeviceSynchronize();
    hipFree(d_pid);
    hipFree(d_counts);
    return e == hipSuccess ? 0 : 1;
}
