/* arroyo-amd non-windowed (TTL'd) stream-stream join: MI355X-native
 * (gfx950) equivalent of JoinWithExpiration
 * (crates/arroyo-worker/src/arrow/join_with_expiration.rs) behind the
 * arroyo_amd_expjoin_* C ABI (include/arroyo_amd.h).
 *
 * MI355X-first design (NOT a translation of the reference's per-key
 * RecordBatch map + per-pair DataFusion HashJoinExec):
 *   - Per side, the stored state is a device-resident chained hash multimap:
 *     an open-addressing key table (CAS-claimed, never un-claimed) whose
 *     chains link rows in an append-only pool (vals SoA + ts + next).  This
 *     replaces KeyTimeView's HashMap<row, Vec<RecordBatch>>
 *     (expiring_time_key_map.rs:932-1050) with a layout a probe wavefront
 *     can walk with coalesced pool reads.
 *   - process_batch = two kernels on one stream: k_ej_probe streams the
 *     incoming rows against the OTHER side's map and emits matched pairs
 *     [key, left vals, right vals, max(ts_l, ts_r)] through a global output
 *     cursor (the reference's compute_pair + post-join max-timestamp
 *     projection, join_with_expiration.rs:110-130 +
 *     arroyo-planner/src/plan/join.rs:121-191), then k_ej_insert appends the
 *     batch into its OWN side's map.  Probe-before-insert on one stream
 *     reproduces the reference's emit-once-when-the-later-row-arrives
 *     semantics exactly (same-side rows never join each other).
 *   - The live map never evicts during a run — matching the reference,
 *     whose in-memory KeyTimeView has no TTL path (table_manager.rs:533;
 *     TTL filters only checkpoint restore).  arroyo_amd_expjoin_expire()
 *     applies the restore cutoff (watermark - ttl) explicitly by rebuilding
 *     the live rows into a fresh pool (k_ej_compact), giving the
 *     bounded-memory mode a production deployment needs.
 *
 * Parity is pinned against oracle/arroyo_oracle.c (itself pinned against
 * the reference's updating_inner_join golden vector) by
 * tests/test_expjoin.py.
 */
#include <hipcub/hipcub.hpp>

#include "op_common.h"

namespace ejoin {

#define EJERR_TABLE_FULL 1
#define EJERR_POOL_FULL  2
#define EJERR_OUT_CAP    3
#define EJERR_RETRACT    4

/* one side's device state */
struct SideMap {
    int64_t *keys;      /* [C] open addressing; spec head for key==-1 */
    int32_t *head;      /* [C+1] chain heads (-1 empty); [C] = spec */
    int32_t *next;      /* [R] */
    int64_t *vals;      /* [nv][R] */
    int64_t *ts;        /* [R] */
    int32_t *cnt;       /* [C+1] live rows per key (updating/outer modes) */
    unsigned long long *cursor; /* pool allocation */
    uint32_t C;
    int64_t R;
    int32_t nv;
};

__device__ inline int64_t find_slot(const SideMap &S, int64_t key) {
    if (key == EMPTY_KEY) return (int64_t)S.C;
    uint64_t m = S.C - 1;
    uint64_t j = hash64((uint64_t)key) & m;
    for (uint32_t probes = 0; probes < S.C; probes++) {
        int64_t cur = S.keys[j];
        if (cur == key) return (int64_t)j;
        if (cur == EMPTY_KEY) return -1;
        j = (j + 1) & m;
    }
    return -1;
}

__device__ inline int64_t claim_slot(const SideMap &S, int64_t key,
                                     int *err) {
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
    *err = EJERR_TABLE_FULL;
    return -1;
}

struct ProbeArgs {
    const int64_t *cols[12];  /* key, vals..., ts of the incoming batch */
    int32_t nv;               /* incoming side's value count */
    int64_t n_rows;
    int32_t side;             /* 0 = incoming is left */
    SideMap other;
    int64_t *out[16];         /* [key, lvals, rvals, ts] */
    unsigned long long *n_out;
    int64_t out_cap;
    int *err;
};

__global__ void __launch_bounds__(256)
k_ej_probe(ProbeArgs P) {
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t *ts = P.cols[1 + P.nv];
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         r < P.n_rows; r += stride) {
        int64_t key = P.cols[0][r];
        int64_t slot = find_slot(P.other, key);
        if (slot < 0) continue;
        /* every row in a slot's chain carries that slot's key (one slot per
         * key; the spec chain holds only key == -1 rows) */
        for (int32_t j = P.other.head[slot]; j >= 0; j = P.other.next[j]) {
            int64_t o = (int64_t)atomicAdd(P.n_out, 1ULL);
            if (o >= P.out_cap) { *P.err = EJERR_OUT_CAP; continue; }
            int col = 0;
            P.out[col++][o] = key;
            if (P.side == 0) {
                for (int v = 0; v < P.nv; v++)
                    P.out[col++][o] = P.cols[1 + v][r];
                for (int v = 0; v < P.other.nv; v++)
                    P.out[col++][o] = P.other.vals[(size_t)v * P.other.R + j];
            } else {
                for (int v = 0; v < P.other.nv; v++)
                    P.out[col++][o] = P.other.vals[(size_t)v * P.other.R + j];
                for (int v = 0; v < P.nv; v++)
                    P.out[col++][o] = P.cols[1 + v][r];
            }
            int64_t ot = P.other.ts[j];
            P.out[col][o] = ts[r] > ot ? ts[r] : ot;
        }
    }
}

struct InsertArgs {
    const int64_t *cols[12];
    int32_t nv;
    int64_t n_rows;
    SideMap own;
    int *err;
};

__global__ void __launch_bounds__(256)
k_ej_insert(InsertArgs I) {
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t *ts = I.cols[1 + I.nv];
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         r < I.n_rows; r += stride) {
        int64_t key = I.cols[0][r];
        int64_t slot = claim_slot(I.own, key, I.err);
        if (slot < 0) continue;
        int64_t idx = (int64_t)atomicAdd(I.own.cursor, 1ULL);
        if (idx >= I.own.R) { *I.err = EJERR_POOL_FULL; continue; }
        for (int v = 0; v < I.nv; v++)
            I.own.vals[(size_t)v * I.own.R + idx] = I.cols[1 + v][r];
        I.own.ts[idx] = ts[r];
        I.own.next[idx] = atomicExch(&I.own.head[slot], (int32_t)idx);
        atomicAdd(&I.own.cnt[slot], 1);
    }
}

/* expire: rebuild each chain into a fresh pool keeping rows with
 * ts >= cutoff; one thread per key slot (chains are per-key: no races) */
struct CompactArgs {
    SideMap src;
    SideMap dst;              /* same keys array; fresh head/next/pool */
    uint64_t cutoff;
    int *err;
};

__global__ void __launch_bounds__(256)
k_ej_compact(CompactArgs A) {
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t slot = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         slot <= (int64_t)A.src.C; slot += stride) {
        if (slot < (int64_t)A.src.C && A.src.keys[slot] == EMPTY_KEY)
            continue;
        int32_t kept = 0;
        for (int32_t j = A.src.head[slot]; j >= 0; j = A.src.next[j]) {
            if ((uint64_t)A.src.ts[j] < A.cutoff) continue;
            int64_t idx = (int64_t)atomicAdd(A.dst.cursor, 1ULL);
            if (idx >= A.dst.R) { *A.err = EJERR_POOL_FULL; continue; }
            for (int v = 0; v < A.src.nv; v++)
                A.dst.vals[(size_t)v * A.dst.R + idx] =
                    A.src.vals[(size_t)v * A.src.R + j];
            A.dst.ts[idx] = A.src.ts[j];
            A.dst.next[idx] = atomicExch(&A.dst.head[slot], (int32_t)idx);
            kept++;
        }
        A.dst.cnt[slot] = kept;
    }
}

/* checkpoint drain: one thread per key slot appends its chain's rows */
struct EDrainArgs {
    SideMap side;
    int64_t *out[12];         /* [key, vals..., ts] */
    unsigned long long *n_out;
    int64_t out_cap;
    int *err;
};

__global__ void __launch_bounds__(256)
k_ej_drain(EDrainArgs D) {
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t slot = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         slot <= (int64_t)D.side.C; slot += stride) {
        int64_t key = slot == (int64_t)D.side.C ? EMPTY_KEY
                                                : D.side.keys[slot];
        if (slot < (int64_t)D.side.C && key == EMPTY_KEY) continue;
        for (int32_t j = D.side.head[slot]; j >= 0; j = D.side.next[j]) {
            int64_t o = (int64_t)atomicAdd(D.n_out, 1ULL);
            if (o >= D.out_cap) { *D.err = EJERR_OUT_CAP; continue; }
            int col = 0;
            D.out[col++][o] = key;
            for (int v = 0; v < D.side.nv; v++)
                D.out[col++][o] = D.side.vals[(size_t)v * D.side.R + j];
            D.out[col][o] = D.side.ts[j];
        }
    }
}

/* ------------------------------------------------------------------ */
/* Updating (retraction-carrying) and LEFT/RIGHT/FULL outer modes
 * (join_with_expiration.rs:29-131 with the planner's join_type,
 * plan/join.rs:326-379).  Semantics restated from the CPU oracle
 * (oracle/arroyo_oracle.c expjoin_insert), which is pinned by the
 * reference's updating_left/right/full_join goldens: a key's first match
 * retracts its earlier null-padded row; a retraction removing a key's
 * last match brings the null rows back.
 *
 * Emission order within a key is semantically significant (own-count
 * transitions decide null-row retractions), so the batch is grouped by
 * key — claim the own-side slot per row, radix-sort (slot << 32 | row)
 * — and ONE thread replays each key's rows in row order.  Keys are
 * independent; the other side's map is read-only during a batch, so
 * there are no cross-thread races. */

__global__ void __launch_bounds__(256)
k_ej_slots(const int64_t *keys_col, int64_t n_rows, SideMap own,
           uint64_t *sortkey, int *err) {
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         r < n_rows; r += stride) {
        int64_t slot = claim_slot(own, keys_col[r], err);
        if (slot < 0) slot = own.C;  /* table full: err already set */
        sortkey[r] = ((uint64_t)slot << 32) | (uint32_t)r;
    }
}

__global__ void __launch_bounds__(256)
k_ej_segs(const uint64_t *sorted, int64_t n, uint32_t *segs,
          unsigned int *n_segs) {
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += stride)
        if (i == 0 || (sorted[i] >> 32) != (sorted[i - 1] >> 32))
            segs[atomicAdd(n_segs, 1u)] = (uint32_t)i;
}

/* one output row; lv/rv null => that side absent (oracle eemit2) */
__device__ inline void ej_emit(int64_t *const *out,
                               unsigned long long *n_out, int64_t out_cap,
                               int *err, int nlv, int nrv, int jt, int upd,
                               int64_t key, const int64_t *lv, int64_t lts,
                               const int64_t *rv, int64_t rts, int retract) {
    int64_t o = (int64_t)atomicAdd(n_out, 1ULL);
    if (o >= out_cap) { *err = EJERR_OUT_CAP; return; }
    int col = 0;
    out[col++][o] = key;
    for (int v = 0; v < nlv; v++) out[col++][o] = lv ? lv[v] : 0;
    for (int v = 0; v < nrv; v++) out[col++][o] = rv ? rv[v] : 0;
    out[col++][o] = lv ? (rv ? (lts > rts ? lts : rts) : lts) : rts;
    if (jt != AMD_JOIN_INNER) {
        out[col++][o] = lv != nullptr;
        out[col++][o] = rv != nullptr;
    }
    if (jt != AMD_JOIN_INNER || upd) out[col][o] = retract;
}

struct EjUpdArgs {
    const int64_t *cols[12];   /* key, vals..., [is_retract,] ts */
    int32_t nv, upd, jt, side, nlv, nrv;
    int64_t n_rows;
    const uint64_t *sorted;
    const uint32_t *segs;
    const unsigned int *n_segs;
    SideMap own, other;
    int64_t *out[20];
    unsigned long long *n_out;
    int64_t out_cap;
    int *err;
};

__global__ void __launch_bounds__(256)
k_ej_upd(EjUpdArgs U) {
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t *ts_col = U.cols[1 + U.nv + U.upd];
    const int64_t *retr_col = U.upd ? U.cols[1 + U.nv] : nullptr;
    const int null_own =
        U.jt == AMD_JOIN_FULL ||
        (U.side == 0 ? U.jt == AMD_JOIN_LEFT : U.jt == AMD_JOIN_RIGHT);
    const int null_other =
        U.jt == AMD_JOIN_FULL ||
        (U.side == 0 ? U.jt == AMD_JOIN_RIGHT : U.jt == AMD_JOIN_LEFT);
    const unsigned int nseg = *U.n_segs;
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         g < (int64_t)nseg; g += stride) {
        int64_t i0 = U.segs[g];
        const int64_t slot = (int64_t)(U.sorted[i0] >> 32);
        int32_t cnt_own = U.own.cnt[slot];
        for (int64_t i = i0;
             i < U.n_rows && (int64_t)(U.sorted[i] >> 32) == slot; i++) {
            int64_t r = (int64_t)(uint32_t)U.sorted[i];
            int64_t key = U.cols[0][r];
            int64_t ts = ts_col[r];
            int64_t mine[8];
            for (int v = 0; v < U.nv; v++) mine[v] = U.cols[1 + v][r];
            /* other side: read-only this batch */
            int64_t oslot = find_slot(U.other, key);
            int32_t on = oslot >= 0 ? U.other.cnt[oslot] : 0;
            int32_t ohead = (oslot >= 0 && on > 0) ? U.other.head[oslot] : -1;
            int64_t ovals[8];
            const int retr = retr_col ? (int)retr_col[r] : 0;
            if (!retr) {
                if (on > 0) {
                    for (int32_t j = ohead; j >= 0; j = U.other.next[j]) {
                        for (int v = 0; v < U.other.nv; v++)
                            ovals[v] =
                                U.other.vals[(size_t)v * U.other.R + j];
                        int64_t ots = U.other.ts[j];
                        if (U.side == 0)
                            ej_emit(U.out, U.n_out, U.out_cap, U.err,
                                    U.nlv, U.nrv, U.jt, U.upd, key, mine,
                                    ts, ovals, ots, 0);
                        else
                            ej_emit(U.out, U.n_out, U.out_cap, U.err,
                                    U.nlv, U.nrv, U.jt, U.upd, key, ovals,
                                    ots, mine, ts, 0);
                    }
                    if (null_other && cnt_own == 0)
                        /* the other side's rows were unmatched until now:
                         * retract their null-padded emissions */
                        for (int32_t j = ohead; j >= 0; j = U.other.next[j]) {
                            for (int v = 0; v < U.other.nv; v++)
                                ovals[v] =
                                    U.other.vals[(size_t)v * U.other.R + j];
                            int64_t ots = U.other.ts[j];
                            if (U.side == 0)
                                ej_emit(U.out, U.n_out, U.out_cap, U.err,
                                        U.nlv, U.nrv, U.jt, U.upd, key,
                                        nullptr, 0, ovals, ots, 1);
                            else
                                ej_emit(U.out, U.n_out, U.out_cap, U.err,
                                        U.nlv, U.nrv, U.jt, U.upd, key,
                                        ovals, ots, nullptr, 0, 1);
                        }
                } else if (null_own) {
                    if (U.side == 0)
                        ej_emit(U.out, U.n_out, U.out_cap, U.err, U.nlv,
                                U.nrv, U.jt, U.upd, key, mine, ts, nullptr,
                                0, 0);
                    else
                        ej_emit(U.out, U.n_out, U.out_cap, U.err, U.nlv,
                                U.nrv, U.jt, U.upd, key, nullptr, 0, mine,
                                ts, 0);
                }
                /* append to own chain (single writer for this slot) */
                int64_t idx = (int64_t)atomicAdd(U.own.cursor, 1ULL);
                if (idx >= U.own.R) { *U.err = EJERR_POOL_FULL; continue; }
                for (int v = 0; v < U.nv; v++)
                    U.own.vals[(size_t)v * U.own.R + idx] = mine[v];
                U.own.ts[idx] = ts;
                U.own.next[idx] = U.own.head[slot];
                U.own.head[slot] = (int32_t)idx;
                cnt_own++;
            } else {
                /* retract: unlink the OLDEST value-equal stored row (the
                 * chain is LIFO, so the last match along the walk) */
                int32_t prev = -1, match = -1, mprev = -1;
                for (int32_t j = U.own.head[slot]; j >= 0;
                     prev = j, j = U.own.next[j]) {
                    int eq = 1;
                    for (int v = 0; v < U.nv && eq; v++)
                        eq = U.own.vals[(size_t)v * U.own.R + j] == mine[v];
                    if (eq) { match = j; mprev = prev; }
                }
                if (match < 0) { *U.err = EJERR_RETRACT; continue; }
                int64_t sts = U.own.ts[match];
                if (on > 0) {
                    for (int32_t j = ohead; j >= 0; j = U.other.next[j]) {
                        for (int v = 0; v < U.other.nv; v++)
                            ovals[v] =
                                U.other.vals[(size_t)v * U.other.R + j];
                        int64_t ots = U.other.ts[j];
                        if (U.side == 0)
                            ej_emit(U.out, U.n_out, U.out_cap, U.err,
                                    U.nlv, U.nrv, U.jt, U.upd, key, mine,
                                    sts, ovals, ots, 1);
                        else
                            ej_emit(U.out, U.n_out, U.out_cap, U.err,
                                    U.nlv, U.nrv, U.jt, U.upd, key, ovals,
                                    ots, mine, sts, 1);
                    }
                    if (null_other && cnt_own == 1)
                        /* the other side loses its last match: null rows
                         * come back */
                        for (int32_t j = ohead; j >= 0; j = U.other.next[j]) {
                            for (int v = 0; v < U.other.nv; v++)
                                ovals[v] =
                                    U.other.vals[(size_t)v * U.other.R + j];
                            int64_t ots = U.other.ts[j];
                            if (U.side == 0)
                                ej_emit(U.out, U.n_out, U.out_cap, U.err,
                                        U.nlv, U.nrv, U.jt, U.upd, key,
                                        nullptr, 0, ovals, ots, 0);
                            else
                                ej_emit(U.out, U.n_out, U.out_cap, U.err,
                                        U.nlv, U.nrv, U.jt, U.upd, key,
                                        ovals, ots, nullptr, 0, 0);
                        }
                } else if (null_own) {
                    if (U.side == 0)
                        ej_emit(U.out, U.n_out, U.out_cap, U.err, U.nlv,
                                U.nrv, U.jt, U.upd, key, mine, sts, nullptr,
                                0, 1);
                    else
                        ej_emit(U.out, U.n_out, U.out_cap, U.err, U.nlv,
                                U.nrv, U.jt, U.upd, key, nullptr, 0, mine,
                                sts, 1);
                }
                if (mprev < 0)
                    U.own.head[slot] = U.own.next[match];
                else
                    U.own.next[mprev] = U.own.next[match];
                cnt_own--;
            }
        }
        U.own.cnt[slot] = cnt_own;
    }
}

}  // namespace ejoin

using namespace ejoin;

struct GpuExpJoin : OpBase {
    AmdExpJoinConfig cfg;
    SideMap side[2];
    /* updating/outer-mode scratch: per-batch (slot<<32|row) sort + key
     * segments (see k_ej_upd) */
    uint64_t *d_sortin = nullptr, *d_sortout = nullptr;
    uint32_t *d_segs = nullptr;
    unsigned int *d_nseg = nullptr;
    void *d_ejtmp = nullptr;
    size_t ejtmp_bytes = 0;
    int64_t *d_out[16];
    unsigned long long *d_n_out;
    Staging stg;
    int out_cols;
    int64_t out_cap;
    int has_wm; uint64_t wm;
};

/* everything of a side but its key table: what expire() rebuilds */
static hipError_t ej_alloc_chains(GpuExpJoin *o, SideMap *S) {
    size_t C1 = (size_t)S->C + 1, R = (size_t)S->R;
    hipError_t e = o->dev_alloc(S->head, C1 * 4, 0xFF);
    if (!e) e = o->dev_alloc(S->next, R * 4);
    if (!e) e = o->dev_alloc(S->vals, (size_t)(S->nv ? S->nv : 1) * R * 8);
    if (!e) e = o->dev_alloc(S->ts, R * 8);
    if (!e) e = o->dev_alloc(S->cnt, C1 * 4, 0);
    if (!e) e = o->dev_alloc(S->cursor, 8, 0);
    return e;
}

static hipError_t ej_alloc_side(GpuExpJoin *o, SideMap *S, uint32_t C,
                                int64_t R, int32_t nv) {
    S->C = C;
    S->R = R;
    S->nv = nv;
    hipError_t e = o->dev_alloc(S->keys, (size_t)C * 8, 0xFF);
    return e ? e : ej_alloc_chains(o, S);
}

API void *arroyo_amd_expjoin_create(const AmdExpJoinConfig *cfg) {
    if (!cfg || cfg->n_keys != 1 || cfg->n_left_vals < 0 ||
        cfg->n_left_vals > 8 || cfg->n_right_vals < 0 ||
        cfg->n_right_vals > 8 || cfg->ttl_nanos == 0) {
        snprintf(g_create_err, sizeof g_create_err, "invalid expjoin config");
        return nullptr;
    }
    if (cfg->join_type < 0 || cfg->join_type > AMD_JOIN_FULL) {
        snprintf(g_create_err, sizeof g_create_err, "invalid join_type");
        return nullptr;
    }
    GpuExpJoin *o = new GpuExpJoin();
    o->cfg = *cfg;
    /* non-inner: + [left_present, right_present]; non-inner or updating:
     * + trailing is_retract (matches oracle_expjoin_create) */
    o->out_cols = 1 + cfg->n_left_vals + cfg->n_right_vals + 1 +
                  (cfg->join_type != AMD_JOIN_INNER ? 2 : 0) +
                  (cfg->join_type != AMD_JOIN_INNER || cfg->updating ? 1 : 0);
    o->out_cap = 1ll << (cfg->log2_out_cap ? cfg->log2_out_cap : 20);
    if (hipSetDevice(cfg->device) != hipSuccess) {
        snprintf(g_create_err, sizeof g_create_err,
                 "hipSetDevice(%d) failed: no HIP device (no CPU fallback)",
                 cfg->device);
        delete o;
        return nullptr;
    }
    uint32_t C = 1u << (cfg->log2_capacity ? cfg->log2_capacity : 16);
    int64_t R = 1ll << (cfg->log2_rows_cap ? cfg->log2_rows_cap : 20);
    for (int s = 0; s < 2; s++)
        OP_TRY(o, "expjoin alloc",
               ej_alloc_side(o, &o->side[s], C, R,
                             s == 0 ? cfg->n_left_vals : cfg->n_right_vals));
    for (int i = 0; i < o->out_cols; i++)
        OP_TRY(o, "expjoin alloc",
               o->dev_alloc(o->d_out[i], (size_t)o->out_cap * 8));
    /* the device-resident ingest path accumulates matches from a cursor
     * that must start at zero (the host path resets it per batch, which
     * masked a reused allocation's stale value here) */
    OP_TRY(o, "expjoin alloc", o->dev_alloc(o->d_n_out, 8, 0));
    OP_TRY(o, "expjoin alloc", o->dev_alloc(o->d_err, 4, 0));
    OP_TRY(o, "hipStreamCreate", o->stream_create(&o->stream));
    int max_in = 1 + (cfg->n_left_vals > cfg->n_right_vals
                          ? cfg->n_left_vals
                          : cfg->n_right_vals) +
                 (cfg->updating ? 1 : 0) + 1;
    OP_TRY_MSG(o, "expjoin staging alloc failed",
               o->stg.alloc(o, max_in, 1 << 20));
    return o;
}

API const char *arroyo_amd_expjoin_last_error(void *h) {
    return h ? ((GpuExpJoin *)h)->err_msg : g_create_err;
}

/* Arrow validity bitmaps for the updating/outer output's null-padded
 * value columns ([key, lvals, rvals, ts, lp, rp, retract]) */
static int ej_fill_validity(GpuExpJoin *o, AmdOutBatch *out) {
    if (o->cfg.join_type == AMD_JOIN_INNER) return 0;
    int nlv = o->cfg.n_left_vals, nrv = o->cfg.n_right_vals;
    int lp = 1 + nlv + nrv + 1;
    int64_t n = out->n_rows;
    bool oom = out_alloc_validity(out);
    for (int g = 0; n && !oom && g < 2; g++) {
        int base = g == 0 ? 1 : 1 + nlv;
        int cnt = g == 0 ? nlv : nrv;
        const int64_t *pres = (const int64_t *)out->cols[g == 0 ? lp
                                                                : lp + 1];
        for (int c = base; c < base + cnt && !oom; c++) {
            uint8_t *bm = out_validity_col(out, c);
            if (!bm) { oom = true; break; }
            for (int64_t r = 0; r < n; r++)
                if (pres[r]) bm[r >> 3] |= (uint8_t)(1u << (r & 7));
        }
    }
    if (!oom) return 0;
    out_free_host(out);
    snprintf(o->err_msg, sizeof o->err_msg,
             "validity bitmap allocation failed");
    return 1;
}

static const char *ej_err_msg(int e) {
    return e == EJERR_TABLE_FULL ? "join key table full; raise log2_capacity"
           : e == EJERR_POOL_FULL
               ? "stored-row pool full; raise log2_rows_cap or expire()"
           : e == EJERR_OUT_CAP ? "output buffer full; raise log2_out_cap"
           : e == EJERR_RETRACT ? "retract of unknown row"
                                : "device error";
}

/* updating/outer ingest: group the batch by key, then replay each key's
 * rows in order with one thread (k_ej_upd) */
static int ej_ingest_upd(GpuExpJoin *o, int32_t side,
                         const int64_t *const *dcols, int64_t n_rows) {
    int32_t nv = side == 0 ? o->cfg.n_left_vals : o->cfg.n_right_vals;
    if (!o->d_sortin) {
        HIP_CHECK(o, o->dev_alloc(o->d_sortin, (size_t)o->stg.cap * 8));
        HIP_CHECK(o, o->dev_alloc(o->d_sortout, (size_t)o->stg.cap * 8));
        HIP_CHECK(o, o->dev_alloc(o->d_segs, (size_t)o->stg.cap * 4));
        HIP_CHECK(o, o->dev_alloc(o->d_nseg, 4));
        o->ejtmp_bytes = 0;
        HIP_CHECK(o, hipcub::DeviceRadixSort::SortKeys(
                         nullptr, o->ejtmp_bytes, o->d_sortin, o->d_sortout,
                         (int)o->stg.cap));
        HIP_CHECK(o, o->dev_alloc(o->d_ejtmp,
                                  o->ejtmp_bytes ? o->ejtmp_bytes : 1));
    }
    hipLaunchKernelGGL(k_ej_slots, dim3(grid_for(n_rows, 4096)), dim3(256), 0,
                       o->stream, dcols[0], n_rows, o->side[side],
                       o->d_sortin, o->d_err);
    HIP_CHECK(o, hipGetLastError());
    size_t tmp = o->ejtmp_bytes;
    HIP_CHECK(o, hipcub::DeviceRadixSort::SortKeys(
                     o->d_ejtmp, tmp, o->d_sortin, o->d_sortout, (int)n_rows,
                     0, 64, o->stream));
    HIP_CHECK(o, hipMemsetAsync(o->d_nseg, 0, 4, o->stream));
    hipLaunchKernelGGL(k_ej_segs, dim3(grid_for(n_rows, 4096)), dim3(256), 0,
                       o->stream, o->d_sortout, n_rows, o->d_segs,
                       o->d_nseg);
    HIP_CHECK(o, hipGetLastError());
    EjUpdArgs U = {};
    for (int c = 0; c < 1 + nv + (o->cfg.updating ? 1 : 0) + 1; c++)
        U.cols[c] = dcols[c];
    U.nv = nv;
    U.upd = o->cfg.updating ? 1 : 0;
    U.jt = o->cfg.join_type;
    U.side = side;
    U.nlv = o->cfg.n_left_vals;
    U.nrv = o->cfg.n_right_vals;
    U.n_rows = n_rows;
    U.sorted = o->d_sortout;
    U.segs = o->d_segs;
    U.n_segs = o->d_nseg;
    U.own = o->side[side];
    U.other = o->side[1 - side];
    for (int i = 0; i < o->out_cols; i++) U.out[i] = o->d_out[i];
    U.n_out = o->d_n_out;
    U.out_cap = o->out_cap;
    U.err = o->d_err;
    hipLaunchKernelGGL(k_ej_upd, dim3(grid_for(n_rows, 4096)), dim3(256), 0,
                       o->stream, U);
    HIP_CHECK(o, hipGetLastError());
    return 0;
}

static int ej_ingest(GpuExpJoin *o, int32_t side, const int64_t *const *dcols,
                     int64_t n_rows, int emit) {
    int32_t nv = side == 0 ? o->cfg.n_left_vals : o->cfg.n_right_vals;
    if (emit && (o->cfg.join_type != AMD_JOIN_INNER || o->cfg.updating))
        return ej_ingest_upd(o, side, dcols, n_rows);
    if (emit) {
        ProbeArgs P = {};
        for (int c = 0; c < 1 + nv + 1; c++) P.cols[c] = dcols[c];
        P.nv = nv;
        P.n_rows = n_rows;
        P.side = side;
        P.other = o->side[1 - side];
        for (int i = 0; i < o->out_cols; i++) P.out[i] = o->d_out[i];
        P.n_out = o->d_n_out;
        P.out_cap = o->out_cap;
        P.err = o->d_err;
        hipLaunchKernelGGL(k_ej_probe, dim3(grid_for(n_rows, 4096)),
                           dim3(256), 0,
                           o->stream, P);
        HIP_CHECK(o, hipGetLastError());
    }
    InsertArgs I = {};
    for (int c = 0; c < 1 + nv + 1; c++) I.cols[c] = dcols[c];
    I.nv = nv;
    I.n_rows = n_rows;
    I.own = o->side[side];
    I.err = o->d_err;
    hipLaunchKernelGGL(k_ej_insert, dim3(grid_for(n_rows, 4096)), dim3(256), 0,
                       o->stream, I);
    HIP_CHECK(o, hipGetLastError());
    return 0;
}

static int ej_copy_in(GpuExpJoin *o, int32_t side,
                      const int64_t *const *cols, int32_t n_cols,
                      int64_t n_rows, int emit, uint64_t cutoff) {
    int64_t done = 0;
    while (done < n_rows) {
        int64_t take = n_rows - done;
        if (take > o->stg.cap) take = o->stg.cap;
        const int64_t *dcols[12];
        if (cutoff) {
            /* restore-time TTL filter: keep ts >= cutoff */
            const int64_t *ts = cols[n_cols - 1];
            int64_t w = 0;
            for (int64_t i = 0; i < take; i++) {
                if ((uint64_t)ts[done + i] < cutoff) continue;
                for (int c = 0; c < n_cols; c++)
                    o->stg.h[c][w] = cols[c][done + i];
                w++;
            }
            if (w && (o->stg.upload(o, n_cols, w, dcols) ||
                      ej_ingest(o, side, dcols, w, emit)))
                return 1;
        } else if (o->stg.stage_chunk(o, cols, n_cols, done, take, dcols) ||
                   ej_ingest(o, side, dcols, take, emit)) {
            return 1;
        }
        HIP_CHECK(o, hipStreamSynchronize(o->stream));
        done += take;
    }
    return 0;
}

/* the first n rows of d_out as a host batch, with the outer-join bitmaps */
static int ej_out(GpuExpJoin *o, AmdOutBatch *out, int64_t n, int n_cols,
                  const char *who) {
    return op_out_alloc(o, out, n, n_cols, who) ||
           out_copy_cols(o, out, o->d_out, n) || ej_fill_validity(o, out);
}

API int arroyo_amd_expjoin_process_batch(void *h, int32_t side,
                                         const int64_t *const *cols,
                                         int32_t n_cols, int64_t n_rows,
                                         AmdOutBatch *out) {
    GpuExpJoin *o = (GpuExpJoin *)h;
    int32_t nv = side == 0 ? o->cfg.n_left_vals : o->cfg.n_right_vals;
    int want = 1 + nv + (o->cfg.updating ? 1 : 0) + 1;
    if (n_cols != want) {
        snprintf(o->err_msg, sizeof o->err_msg, "side %d expects %d cols",
                 side, want);
        return 1;
    }
    HIP_CHECK(o, hipMemsetAsync(o->d_n_out, 0, 8, o->stream));
    if (ej_copy_in(o, side, cols, n_cols, n_rows, 1, 0)) return 1;
    unsigned long long n = 0;
    HIP_CHECK(o, hipMemcpyAsync(&n, o->d_n_out, 8, hipMemcpyDeviceToHost,
                                o->stream));
    HIP_CHECK(o, hipStreamSynchronize(o->stream));
    if (op_check_err(o, ej_err_msg)) return 1;
    if (out && ej_out(o, out, (int64_t)n, o->out_cols, __func__)) return 1;
    return 0;
}

/* device-resident ingest: probes + inserts without host staging; matched
 * rows stay in d_out (the n_out cursor is NOT reset here so several
 * device batches may accumulate until expjoin_collect drains them) */
API int arroyo_amd_expjoin_process_batch_device(void *h, int32_t side,
                                                const int64_t *const *dcols,
                                                int32_t n_cols,
                                                int64_t n_rows) {
    GpuExpJoin *o = (GpuExpJoin *)h;
    int32_t nv = side == 0 ? o->cfg.n_left_vals : o->cfg.n_right_vals;
    int want = 1 + nv + (o->cfg.updating ? 1 : 0) + 1;
    if (n_cols != want) {
        snprintf(o->err_msg, sizeof o->err_msg, "side %d expects %d cols",
                 side, want);
        return 1;
    }
    return ej_ingest(o, side, dcols, n_rows, 1);
}

/* drain the accumulated device-side match rows to the host */
API int arroyo_amd_expjoin_collect(void *h, AmdOutBatch *out) {
    GpuExpJoin *o = (GpuExpJoin *)h;
    unsigned long long n = 0;
    HIP_CHECK(o, hipMemcpyAsync(&n, o->d_n_out, 8, hipMemcpyDeviceToHost,
                                o->stream));
    HIP_CHECK(o, hipStreamSynchronize(o->stream));
    if (op_check_err(o, ej_err_msg)) return 1;
    if (ej_out(o, out, (int64_t)n, o->out_cols, __func__)) return 1;
    HIP_CHECK(o, hipMemsetAsync(o->d_n_out, 0, 8, o->stream));
    return 0;
}

/* device-resident consumption: report and reset the accumulated match
 * count without copying the match columns to the host (the next pipeline
 * stage consumes d_out in place -- the same accounting convention as the
 * window operator's emitted-rows accumulator) */
API int arroyo_amd_expjoin_match_count(void *h, int64_t *n_matches) {
    GpuExpJoin *o = (GpuExpJoin *)h;
    unsigned long long n = 0;
    HIP_CHECK(o, hipMemcpyAsync(&n, o->d_n_out, 8, hipMemcpyDeviceToHost,
                                o->stream));
    HIP_CHECK(o, hipStreamSynchronize(o->stream));
    if (op_check_err(o, ej_err_msg)) return 1;
    *n_matches = (int64_t)n;
    HIP_CHECK(o, hipMemsetAsync(o->d_n_out, 0, 8, o->stream));
    return 0;
}

API int arroyo_amd_expjoin_handle_watermark(void *h, uint64_t wm) {
    GpuExpJoin *o = (GpuExpJoin *)h;
    o->has_wm = 1;
    o->wm = wm;
    return op_check_err(o, ej_err_msg);
}

API int arroyo_amd_expjoin_expire(void *h) {
    GpuExpJoin *o = (GpuExpJoin *)h;
    if (!o->has_wm || o->wm < o->cfg.ttl_nanos) return 0;
    uint64_t cutoff = o->wm - o->cfg.ttl_nanos;
    for (int s = 0; s < 2; s++) {
        SideMap *S = &o->side[s];
        SideMap fresh = *S;  /* key table survives; chains rebuilt */
        HIP_CHECK(o, ej_alloc_chains(o, &fresh));
        CompactArgs A = {};
        A.src = *S;
        A.dst = fresh;
        A.cutoff = cutoff;
        A.err = o->d_err;
        hipLaunchKernelGGL(k_ej_compact,
                           dim3(grid_for((int64_t)S->C + 1, 4096)),
                           dim3(256), 0, o->stream, A);
        HIP_CHECK(o, hipGetLastError());
        HIP_CHECK(o, hipStreamSynchronize(o->stream));
        o->release(S->head);
        o->release(S->next);
        o->release(S->vals);
        o->release(S->ts);
        o->release(S->cnt);
        o->release(S->cursor);
        *S = fresh;
    }
    return op_check_err(o, ej_err_msg);
}

API int arroyo_amd_expjoin_checkpoint_drain(void *h, int32_t side,
                                            AmdOutBatch *out) {
    GpuExpJoin *o = (GpuExpJoin *)h;
    if (op_check_err(o, ej_err_msg)) return 1;
    SideMap *S = &o->side[side];
    int ncols = 1 + S->nv + 1;
    HIP_CHECK(o, hipMemsetAsync(o->d_n_out, 0, 8, o->stream));
    EDrainArgs D = {};
    D.side = *S;
    for (int i = 0; i < ncols; i++) D.out[i] = o->d_out[i];
    D.n_out = o->d_n_out;
    D.out_cap = o->out_cap;
    D.err = o->d_err;
    hipLaunchKernelGGL(k_ej_drain, dim3(grid_for((int64_t)S->C + 1, 4096)),
                       dim3(256), 0, o->stream, D);
    HIP_CHECK(o, hipGetLastError());
    unsigned long long n = 0;
    HIP_CHECK(o, hipMemcpyAsync(&n, o->d_n_out, 8, hipMemcpyDeviceToHost,
                                o->stream));
    HIP_CHECK(o, hipStreamSynchronize(o->stream));
    if (op_check_err(o, ej_err_msg)) return 1;
    return op_out_alloc(o, out, (int64_t)n, ncols, __func__) ||
           out_copy_cols(o, out, o->d_out, (int64_t)n);
}

API int arroyo_amd_expjoin_restore(void *h, int32_t side,
                                   const int64_t *const *cols,
                                   int32_t n_cols, int64_t n_rows,
                                   int has_watermark,
                                   uint64_t watermark_nanos) {
    GpuExpJoin *o = (GpuExpJoin *)h;
    int32_t nv = side == 0 ? o->cfg.n_left_vals : o->cfg.n_right_vals;
    if (n_cols != 1 + nv + 1) {
        snprintf(o->err_msg, sizeof o->err_msg, "side %d expects %d cols",
                 side, 1 + nv + 1);
        return 1;
    }
    uint64_t cutoff = 0;
    if (has_watermark && watermark_nanos > o->cfg.ttl_nanos)
        cutoff = watermark_nanos - o->cfg.ttl_nanos;
    if (ej_copy_in(o, side, cols, n_cols, n_rows, 0,
                   cutoff ? cutoff : 0))
        return 1;
    /* carry the restored watermark so a post-restore expire() uses it
     * (documented restore semantics; was a silent no-op until the next
     * handle_watermark) */
    if (has_watermark) {
        o->has_wm = 1;
        if (watermark_nanos > o->wm) o->wm = watermark_nanos;
    }
    return op_check_err(o, ej_err_msg);
}

API void arroyo_amd_expjoin_destroy(void *h) {
    delete (GpuExpJoin *)h;   /* ~OpBase drains the stream first */
}
