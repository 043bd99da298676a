/* arroyo-amd instant (windowed stream-stream) join, behind the
 * arroyo_amd_join_* C ABI (include/arroyo_amd.h). */
#include <map>

#include "op_common.h"

/* ================================================================== */
/* Instant (windowed stream-stream) join: MI355X-native equivalent of
 * InstantJoin (crates/arroyo-worker/src/arrow/instant_join.rs) behind the
 * arroyo_amd_join_* C ABI (include/arroyo_amd.h).
 *
 * Design (not a translation): instead of per-instant DataFusion exec
 * streams fed through channels (instant_join.rs:86-107), both sides'
 * rows land directly in a device-resident instant table: `instants` slots,
 * each an append buffer per side (key + value columns, SoA).  A fused
 * append kernel (K2-equivalent routing + buffering) claims the instant
 * slot by CAS on its tag and appends with a wave-aggregated cursor.  On
 * watermark the host fires instants < wm in timestamp order
 * (instant_join.rs:265-281): per instant, a build kernel chains the left
 * rows into a hash multimap (LDS-free; the map is small and L2-resident)
 * and a probe kernel streams the right rows and emits matches (K6) --
 * or, for n_keys == 0 (join on the window itself), a cross-product
 * kernel with no atomics at all. */

#define JERR_LATE      4
#define JERR_INSTANTS  5
#define JERR_ROWS_CAP  6
#define JERR_OUT_CAP   7

struct JAppendArgs {
    const int64_t *cols[6];   /* key?, vals..., ts */
    int32_t n_keys, n_vals;
    int64_t n_rows;
    uint64_t *tag;            /* [I] */
    unsigned long long *cursor; /* [I] */
    int64_t *key;             /* [I*cap] */
    int64_t *vals;            /* [n_vals][I*cap] */
    uint32_t I, cap;
    int has_wm; uint64_t wm;
    int *err;
};

/* claim-or-find the slot for instant t (open addressing over the tags) */
__device__ inline int32_t claim_instant(uint64_t *tag, uint32_t I, uint64_t t,
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
    *err = JERR_INSTANTS;
    return -1;
}

__global__ void __launch_bounds__(256)
k_join_append(JAppendArgs A) {
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t *ts = A.cols[A.n_keys + A.n_vals];
    int lane = (int)(threadIdx.x & 63);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         i < A.n_rows; i += stride) {
        uint64_t t = (uint64_t)ts[i];
        if (A.has_wm && t < A.wm) { *A.err = JERR_LATE; continue; }
        /* wave-uniform fast path: one leader claims slot + cursor range */
        unsigned long long act = __ballot(1);
        int leader = (int)(__ffsll((long long)act) - 1);
        uint64_t t0 = (uint64_t)__shfl((long long)t, leader, 64);
        int32_t slot;
        uint64_t idx;
        if (__all(t == t0)) {
            int cnt = __popcll((long long)act);
            int rank = __popcll((long long)(act & ((1ULL << lane) - 1)));
            unsigned long long base = 0;
            int32_t s0 = -1;
            if (lane == leader) {
                s0 = claim_instant(A.tag, A.I, t, A.err);
                if (s0 >= 0)
                    base = atomicAdd(&A.cursor[s0], (unsigned long long)cnt);
            }
            slot = (int32_t)__shfl((int)s0, leader, 64);
            base = (unsigned long long)__shfl((long long)base, leader, 64);
            if (slot < 0) continue;
            idx = base + (uint64_t)rank;
        } else {
            slot = claim_instant(A.tag, A.I, t, A.err);
            if (slot < 0) continue;
            idx = atomicAdd(&A.cursor[slot], 1ULL);
        }
        if (idx >= A.cap) { *A.err = JERR_ROWS_CAP; continue; }
        size_t off = (size_t)slot * A.cap + idx;
        int c = 0;
        if (A.n_keys) A.key[off] = A.cols[c++][i];
        for (int v = 0; v < A.n_vals; v++)
            A.vals[(size_t)v * A.I * A.cap + off] = A.cols[c++][i];
    }
}

/* build a chained hash multimap over one instant's left rows.  `base` is
 * the slot's global row offset (slot*cap): chain links are global indices so
 * several slots holding the same instant (possible after slot recycling — a
 * retired slot's tag hole lets a later append re-claim an earlier probe
 * position) can be built into ONE map and joined as one logical instant. */
struct JBuildArgs {
    const int64_t *key;   /* left keys of this slot, [nl] */
    int64_t nl;
    int64_t base;         /* slot*cap: global index of this slot's row 0 */
    int64_t *b_keys;      /* [H] open-addressing key table */
    int32_t *b_head;      /* [H] chain heads (-1 empty) */
    int32_t *b_next;      /* [I*cap], indexed by global row index */
    uint32_t H;
    int *err;
};

__global__ void __launch_bounds__(256)
k_join_build(JBuildArgs B) {
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         i < B.nl; i += stride) {
        int64_t key = B.key[i];
        int64_t s = table_upsert(B.b_keys, B.H, key, B.err);
        if (s < 0) continue;
        B.b_next[B.base + i] =
            atomicExch(&B.b_head[s], (int32_t)(B.base + i));
    }
}

struct JProbeArgs {
    const int64_t *r_key;     /* right keys of this slot, [nr] */
    const int64_t *l_key;     /* left key plane base (global row index) */
    const int64_t *l_vals;    /* [n_left_vals][I*cap] base of left side */
    const int64_t *r_vals;    /* [n_right_vals][I*cap] base of right side */
    size_t l_off, r_off;      /* slot*cap element offset */
    size_t plane;             /* I*cap: stride between value planes */
    int64_t nr;
    const int64_t *b_keys;
    const int32_t *b_head;
    const int32_t *b_next;
    uint32_t H;
    int32_t n_keys, nlv, nrv;
    int32_t jt;               /* AMD_JOIN_* */
    uint32_t *l_hit;          /* [plane/32] matched-left bitmap (outer) */
    uint64_t instant;
    int64_t *out[16];
    unsigned long long *n_out;
    int64_t out_cap;
    int *err;
};

/* li/ri == -1: that side absent (outer join) -> zero-filled values,
 * presence flag 0.  li is a GLOBAL row index when the chain map is in
 * play (l_off = 0), slot-relative otherwise. */
__device__ inline void jemit_row(const JProbeArgs &P, int64_t key, int64_t li,
                                 int64_t ri, int64_t r) {
    if (r >= P.out_cap) { *P.err = JERR_OUT_CAP; return; }
    int col = 0;
    if (P.n_keys) P.out[col++][r] = key;
    for (int v = 0; v < P.nlv; v++)
        P.out[col++][r] =
            li >= 0 ? P.l_vals[(size_t)v * P.plane + P.l_off + li] : 0;
    for (int v = 0; v < P.nrv; v++)
        P.out[col++][r] =
            ri >= 0 ? P.r_vals[(size_t)v * P.plane + P.r_off + ri] : 0;
    P.out[col++][r] = (int64_t)P.instant;
    if (P.jt != AMD_JOIN_INNER) {
        P.out[col++][r] = li >= 0;
        P.out[col][r] = ri >= 0;
    }
}

__global__ void __launch_bounds__(256)
k_join_probe(JProbeArgs P) {
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    uint32_t m = P.H - 1;
    const bool emit_r = P.jt == AMD_JOIN_RIGHT || P.jt == AMD_JOIN_FULL;
    const bool track_l = P.l_hit != nullptr;
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         j < P.nr; j += stride) {
        int64_t key = P.r_key[j];
        uint64_t s = hash64((uint64_t)key) & m;
        int32_t head = -1;
        for (uint32_t probes = 0; probes < P.H; probes++) {
            int64_t k = P.b_keys[s];
            if (k == key) { head = P.b_head[s]; break; }
            if (k == EMPTY_KEY) break;
            s = (s + 1) & m;
        }
        bool hit = false;
        for (int32_t li = head; li >= 0; li = P.b_next[li]) {
            int64_t r = (int64_t)atomicAdd(P.n_out, 1ULL);
            jemit_row(P, key, li, j, r);
            hit = true;
            if (track_l)
                atomicOr(&P.l_hit[(uint32_t)li >> 5], 1u << ((uint32_t)li & 31u));
        }
        if (!hit && emit_r) {
            int64_t r = (int64_t)atomicAdd(P.n_out, 1ULL);
            jemit_row(P, key, -1, j, r);
        }
    }
}

/* pad-every-right-row kernel: window-condition (n_keys == 0) outer joins
 * with an empty left side have no key plane to probe, so emit the right
 * rows directly (slot-relative ri against P.r_off) */
__global__ void __launch_bounds__(256)
k_join_pad_right(JProbeArgs P) {
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t ri = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         ri < P.nr; ri += stride) {
        int64_t r = (int64_t)atomicAdd(P.n_out, 1ULL);
        jemit_row(P, 0, -1, ri, r);
    }
}

/* outer-join left pass: emit every left row of one slot whose matched bit
 * is unset ([base, base+nl) global row indices); with a zeroed bitmap this
 * doubles as the pad-every-left-row kernel for empty-right instants */
__global__ void __launch_bounds__(256)
k_join_unmatched_left(JProbeArgs P, int64_t base, int64_t nl) {
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         i < nl; i += stride) {
        int64_t li = base + i;
        if (P.l_hit[(uint32_t)li >> 5] & (1u << ((uint32_t)li & 31u)))
            continue;
        int64_t r = (int64_t)atomicAdd(P.n_out, 1ULL);
        jemit_row(P, P.n_keys ? P.l_key[li] : 0, li, -1, r);
    }
}

/* n_keys == 0: cross product of the instant's sides, no atomics;
 * `out_base` offsets the output rows so one logical instant spread across
 * several (left slot, right slot) pairs writes disjoint output ranges */
__global__ void __launch_bounds__(256)
k_join_cross(JProbeArgs P, int64_t nl, int64_t out_base) {
    int64_t total = nl * P.nr;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         i < total; i += stride)
        jemit_row(P, 0, i / P.nr, i % P.nr, out_base + i);
}

struct GpuJoin : OpBase {
    AmdJoinConfig cfg;
    uint32_t I, cap, H;
    int64_t out_cap;
    uint64_t *tag;
    unsigned long long *cursor[2];
    int64_t *key[2];
    int64_t *vals[2];          /* [n_vals][I*cap] */
    int64_t *b_keys; int32_t *b_head; int32_t *b_next;
    uint32_t *l_hit;           /* [I*cap/32] matched-left bitmap (outer) */
    int64_t *d_out[16];
    unsigned long long *d_n_out;
    Staging stg[2];            /* host-ingest staging per side */
    std::vector<std::vector<int64_t>> host_out;
    int out_cols;
    int has_wm; uint64_t wm;
    int64_t emitted_device_rows;
};

API void *arroyo_amd_join_create(const AmdJoinConfig *cfg) {
    if (!cfg || cfg->n_keys < 0 || cfg->n_keys > 1 || cfg->n_left_vals < 0 ||
        cfg->n_right_vals < 0 || cfg->n_left_vals > 4 ||
        cfg->n_right_vals > 4 || cfg->join_type < 0 ||
        cfg->join_type > AMD_JOIN_FULL) {
        snprintf(g_create_err, sizeof g_create_err, "invalid join config");
        return nullptr;
    }
    GpuJoin *o = new GpuJoin();
    o->cfg = *cfg;
    o->I = cfg->instants ? cfg->instants : 128;
    o->cap = 1u << (cfg->log2_rows_cap ? cfg->log2_rows_cap : 15);
    o->H = o->cap * 2;
    o->out_cap = 1ll << (cfg->log2_out_cap ? cfg->log2_out_cap : 20);
    o->out_cols = cfg->n_keys + cfg->n_left_vals + cfg->n_right_vals + 1 +
                  (cfg->join_type != AMD_JOIN_INNER ? 2 : 0);
    if (hipSetDevice(cfg->device) != hipSuccess) {
        snprintf(g_create_err, sizeof g_create_err,
                 "hipSetDevice(%d) failed: no HIP device (no CPU fallback)",
                 cfg->device);
        delete o;
        return nullptr;
    }
    size_t plane = (size_t)o->I * o->cap;
    OP_ALLOC(o, o->tag, (size_t)o->I * 8, 0xFF);
    for (int s = 0; s < 2; s++) {
        int nv = s == 0 ? cfg->n_left_vals : cfg->n_right_vals;
        OP_ALLOC(o, o->cursor[s], (size_t)o->I * 8, 0);
        if (cfg->n_keys) OP_ALLOC(o, o->key[s], plane * 8);
        if (nv) OP_ALLOC(o, o->vals[s], (size_t)nv * plane * 8);
    }
    OP_ALLOC(o, o->b_keys, (size_t)o->H * 8);
    OP_ALLOC(o, o->b_head, (size_t)o->H * 4);
    OP_ALLOC(o, o->b_next, (size_t)o->I * o->cap * 4);
    if (cfg->join_type == AMD_JOIN_LEFT || cfg->join_type == AMD_JOIN_FULL)
        OP_ALLOC(o, o->l_hit, plane / 32 * 4 + 4);
    for (int i = 0; i < o->out_cols && i < 16; i++)
        OP_ALLOC(o, o->d_out[i], (size_t)o->out_cap * 8);
    OP_ALLOC(o, o->d_n_out, 8);
    OP_ALLOC(o, o->d_err, 4, 0);
    OP_TRY(o, "hipStreamCreate", o->stream_create(&o->stream));
    for (int s = 0; s < 2; s++) {
        int nv = s == 0 ? cfg->n_left_vals : cfg->n_right_vals;
        OP_TRY_MSG(o, "join staging alloc failed",
                   o->stg[s].alloc(o, cfg->n_keys + nv + 1, 1 << 20));
    }
    o->host_out.resize(o->out_cols);
    return o;
}

API const char *arroyo_amd_join_last_error(void *h) {
    return h ? ((GpuJoin *)h)->err_msg : g_create_err;
}

static const char *join_err_msg(int e) {
    return e == JERR_LATE       ? "batch timestamp before watermark"
           : e == JERR_INSTANTS ? "live-instant table full; raise instants"
           : e == JERR_ROWS_CAP
               ? "per-instant row buffer full; raise log2_rows_cap"
           : e == JERR_OUT_CAP   ? "output buffer full; raise log2_out_cap"
           : e == ERR_TABLE_FULL ? "join build table full"
                                 : "device error";
}

static int join_append_device(GpuJoin *o, int side, const int64_t *const *dcols,
                              int64_t n_rows) {
    if (n_rows == 0) return 0;
    JAppendArgs A = {};
    int nv = side == 0 ? o->cfg.n_left_vals : o->cfg.n_right_vals;
    for (int c = 0; c < o->cfg.n_keys + nv + 1; c++) A.cols[c] = dcols[c];
    A.n_keys = o->cfg.n_keys;
    A.n_vals = nv;
    A.n_rows = n_rows;
    A.tag = o->tag;
    A.cursor = o->cursor[side];
    A.key = o->key[side];
    A.vals = o->vals[side];
    A.I = o->I;
    A.cap = o->cap;
    A.has_wm = o->has_wm;
    A.wm = o->wm;
    A.err = o->d_err;
    int blocks = grid_for(n_rows, 1024);
    hipLaunchKernelGGL(k_join_append, dim3(blocks), dim3(256), 0, o->stream, A);
    HIP_CHECK(o, hipGetLastError());
    return 0;
}

API int arroyo_amd_join_process_batch(void *h, int32_t side,
                                      const int64_t *const *cols,
                                      int32_t n_cols, int64_t n_rows) {
    GpuJoin *o = (GpuJoin *)h;
    int nv = side == 0 ? o->cfg.n_left_vals : o->cfg.n_right_vals;
    if (n_cols != o->cfg.n_keys + nv + 1) {
        snprintf(o->err_msg, sizeof o->err_msg, "side %d expects %d cols",
                 side, o->cfg.n_keys + nv + 1);
        return 1;
    }
    int64_t done = 0;
    while (done < n_rows) {
        int64_t take = n_rows - done;
        if (take > o->stg[side].cap) take = o->stg[side].cap;
        const int64_t *dcols[6];
        if (o->stg[side].stage_chunk(o, cols, n_cols, done, take, dcols) ||
            join_append_device(o, side, dcols, take))
            return 1;
        /* staging reused next iteration: wait for this append to finish */
        HIP_CHECK(o, hipStreamSynchronize(o->stream));
        done += take;
    }
    return 0;
}

API int arroyo_amd_join_process_batch_device(void *h, int32_t side,
                                             const int64_t *const *dcols,
                                             int32_t n_cols, int64_t n_rows) {
    GpuJoin *o = (GpuJoin *)h;
    int nv = side == 0 ? o->cfg.n_left_vals : o->cfg.n_right_vals;
    if (n_cols != o->cfg.n_keys + nv + 1) {
        snprintf(o->err_msg, sizeof o->err_msg, "side %d expects %d cols",
                 side, o->cfg.n_keys + nv + 1);
        return 1;
    }
    return join_append_device(o, side, dcols, n_rows);
}

/* Fire one logical instant.  `slots` is every table slot holding this
 * instant's rows — normally one, but slot recycling can split an instant
 * across slots (see k_join_build comment); the group joins as a whole so no
 * cross-slot match is lost. */
static int join_fire(GpuJoin *o, uint64_t instant,
                     const std::vector<uint32_t> &slots,
                     const std::vector<unsigned long long> &c0,
                     const std::vector<unsigned long long> &c1) {
    size_t plane = (size_t)o->I * o->cap;
    HIP_CHECK(o, hipMemsetAsync(o->d_n_out, 0, 8, o->stream));
    JProbeArgs P = {};
    P.l_vals = o->vals[0];
    P.r_vals = o->vals[1];
    P.plane = plane;
    P.b_keys = o->b_keys;
    P.b_head = o->b_head;
    P.b_next = o->b_next;
    P.H = o->H;
    P.n_keys = o->cfg.n_keys;
    P.nlv = o->cfg.n_left_vals;
    P.nrv = o->cfg.n_right_vals;
    P.jt = o->cfg.join_type;
    P.l_key = o->key[0];
    P.instant = instant;
    for (int i = 0; i < o->out_cols && i < 16; i++) P.out[i] = o->d_out[i];
    P.n_out = o->d_n_out;
    P.out_cap = o->out_cap;
    P.err = o->d_err;
    const bool emit_l =
        P.jt == AMD_JOIN_LEFT || P.jt == AMD_JOIN_FULL;
    const bool emit_r =
        P.jt == AMD_JOIN_RIGHT || P.jt == AMD_JOIN_FULL;
    unsigned long long nl = 0, nr = 0;
    for (uint32_t s : slots) { nl += c0[s]; nr += c1[s]; }
    unsigned long long n = 0;
    auto pad_left_slots = [&](bool use_bitmap) -> int {
        /* emit left rows whose matched bit is unset; with use_bitmap false
         * the bitmap is zeroed first so every row emits (empty right) */
        for (uint32_t ls : slots) {
            if (!c0[ls]) continue;
            int64_t base = (int64_t)ls * o->cap;
            if (!use_bitmap)
                HIP_CHECK(o, hipMemsetAsync(o->l_hit + base / 32, 0,
                                            (size_t)o->cap / 32 * 4,
                                            o->stream));
            JProbeArgs Q = P;
            Q.l_off = 0;
            Q.l_hit = o->l_hit;
            int blocks = grid_for((int64_t)c0[ls], 1024);
            hipLaunchKernelGGL(k_join_unmatched_left, dim3(blocks), dim3(256),
                               0, o->stream, Q, base, (int64_t)c0[ls]);
            HIP_CHECK(o, hipGetLastError());
        }
        return 0;
    };
    if (o->cfg.n_keys == 0) {
        if (nl && nr) {
            int64_t total = (int64_t)nl * (int64_t)nr;
            if (total > o->out_cap) {
                snprintf(o->err_msg, sizeof o->err_msg,
                         "output buffer full; raise log2_out_cap");
                return 1;
            }
            int64_t base = 0;
            for (uint32_t ls : slots) {
                if (!c0[ls]) continue;
                for (uint32_t rs : slots) {
                    if (!c1[rs]) continue;
                    int64_t pair = (int64_t)c0[ls] * (int64_t)c1[rs];
                    P.l_off = (size_t)ls * o->cap;
                    P.r_off = (size_t)rs * o->cap;
                    P.nr = (int64_t)c1[rs];
                    int blocks = grid_for(pair, 1024);
                    hipLaunchKernelGGL(k_join_cross, dim3(blocks), dim3(256),
                                       0, o->stream, P, (int64_t)c0[ls], base);
                    HIP_CHECK(o, hipGetLastError());
                    base += pair;
                }
            }
            n = (unsigned long long)total;
        } else if (nl && emit_l) {
            if (pad_left_slots(false)) return 1;
            HIP_CHECK(o, hipMemcpyAsync(&n, o->d_n_out, 8,
                                        hipMemcpyDeviceToHost, o->stream));
        } else if (nr && emit_r) {
            /* no key plane exists when n_keys == 0: pad the right rows
             * directly instead of probing */
            for (uint32_t rs : slots) {
                if (!c1[rs]) continue;
                P.r_off = (size_t)rs * o->cap;
                P.nr = (int64_t)c1[rs];
                int blocks = grid_for(P.nr, 1024);
                hipLaunchKernelGGL(k_join_pad_right, dim3(blocks), dim3(256),
                                   0, o->stream, P);
                HIP_CHECK(o, hipGetLastError());
            }
            HIP_CHECK(o, hipMemcpyAsync(&n, o->d_n_out, 8,
                                        hipMemcpyDeviceToHost, o->stream));
        }
    } else if ((nl && nr) || (nl && emit_l) || (nr && emit_r)) {
        bool probes = nr && (nl || emit_r);
        if (probes || nl) {
            HIP_CHECK(o, hipMemsetAsync(o->b_keys, 0xFF, (size_t)o->H * 8,
                                        o->stream));
            HIP_CHECK(o, hipMemsetAsync(o->b_head, 0xFF, (size_t)o->H * 4,
                                        o->stream));
        }
        for (uint32_t ls : slots) {
            if (!c0[ls]) continue;
            JBuildArgs B = {};
            B.key = o->key[0] + (size_t)ls * o->cap;
            B.nl = (int64_t)c0[ls];
            B.base = (int64_t)ls * o->cap;
            B.b_keys = o->b_keys;
            B.b_head = o->b_head;
            B.b_next = o->b_next;
            B.H = o->H;
            B.err = o->d_err;
            int blocks = grid_for(B.nl, 1024);
            hipLaunchKernelGGL(k_join_build, dim3(blocks), dim3(256), 0,
                               o->stream, B);
            HIP_CHECK(o, hipGetLastError());
        }
        if (emit_l)
            for (uint32_t ls : slots) {
                if (!c0[ls]) continue;
                HIP_CHECK(o, hipMemsetAsync(
                                 o->l_hit + (size_t)ls * o->cap / 32, 0,
                                 (size_t)o->cap / 32 * 4, o->stream));
            }
        /* chain links are global row indices: probe reads left values at
         * l_vals[v*plane + li] directly, so l_off = 0 */
        P.l_off = 0;
        P.l_hit = emit_l ? o->l_hit : nullptr;
        if (probes)
            for (uint32_t rs : slots) {
                if (!c1[rs]) continue;
                P.r_key = o->key[1] + (size_t)rs * o->cap;
                P.r_off = (size_t)rs * o->cap;
                P.nr = (int64_t)c1[rs];
                int blocks = grid_for(P.nr, 1024);
                hipLaunchKernelGGL(k_join_probe, dim3(blocks), dim3(256), 0,
                                   o->stream, P);
                HIP_CHECK(o, hipGetLastError());
            }
        if (emit_l && nl && pad_left_slots(true)) return 1;
        HIP_CHECK(o, hipMemcpyAsync(&n, o->d_n_out, 8, hipMemcpyDeviceToHost,
                                    o->stream));
    }
    /* retire every slot of the instant */
    for (uint32_t s : slots) {
        HIP_CHECK(o, hipMemsetAsync(o->tag + s, 0xFF, 8, o->stream));
        HIP_CHECK(o, hipMemsetAsync(o->cursor[0] + s, 0, 8, o->stream));
        HIP_CHECK(o, hipMemsetAsync(o->cursor[1] + s, 0, 8, o->stream));
    }
    HIP_CHECK(o, hipStreamSynchronize(o->stream));
    if (n == 0) return 0;
    if ((int64_t)n > o->out_cap) {
        snprintf(o->err_msg, sizeof o->err_msg,
                 "output buffer full; raise log2_out_cap");
        return 1;
    }
    if (o->cfg.emit_to_host) {
        for (int i = 0; i < o->out_cols; i++) {
            size_t old = o->host_out[i].size();
            o->host_out[i].resize(old + n);
            HIP_CHECK(o, hipMemcpyAsync(o->host_out[i].data() + old,
                                        o->d_out[i], (size_t)n * 8,
                                        hipMemcpyDeviceToHost, o->stream));
        }
        HIP_CHECK(o, hipStreamSynchronize(o->stream));
    } else {
        o->emitted_device_rows += (int64_t)n;
    }
    return 0;
}


/* Arrow validity bitmaps for null-padded value columns (LSB bit order,
 * see AmdOutBatch doc): left vals valid where the left-presence column is
 * set, right vals likewise.  The presence columns stay in the output. */
static int fill_join_validity(AmdOutBatch *out, int base_l, int nlv,
                              int nrv, int lp_col, int rp_col) {
    int64_t n = out->n_rows;
    if (out_alloc_validity(out)) return 1;
    for (int g = 0; n && g < 2; g++) {
        int base = g == 0 ? base_l : base_l + nlv;
        int cnt = g == 0 ? nlv : nrv;
        const int64_t *pres =
            (const int64_t *)out->cols[g == 0 ? lp_col : rp_col];
        for (int c = base; c < base + cnt; c++) {
            uint8_t *bm = out_validity_col(out, c);
            if (!bm) return 1;
            for (int64_t r = 0; r < n; r++)
                if (pres[r]) bm[r >> 3] |= (uint8_t)(1u << (r & 7));
        }
    }
    return 0;
}

API int arroyo_amd_join_handle_watermark(void *h, uint64_t wm,
                                         AmdOutBatch *out) {
    GpuJoin *o = (GpuJoin *)h;
    if (op_check_err(o, join_err_msg)) return 1;
    o->has_wm = 1;
    o->wm = wm;
    /* snapshot live instants + row counts */
    std::vector<uint64_t> tags(o->I);
    std::vector<unsigned long long> c0(o->I), c1(o->I);
    HIP_CHECK(o, hipMemcpyAsync(tags.data(), o->tag, (size_t)o->I * 8,
                                hipMemcpyDeviceToHost, o->stream));
    HIP_CHECK(o, hipMemcpyAsync(c0.data(), o->cursor[0], (size_t)o->I * 8,
                                hipMemcpyDeviceToHost, o->stream));
    HIP_CHECK(o, hipMemcpyAsync(c1.data(), o->cursor[1], (size_t)o->I * 8,
                                hipMemcpyDeviceToHost, o->stream));
    HIP_CHECK(o, hipStreamSynchronize(o->stream));
    /* timestamp order (instant_join.rs:265-281); an instant may occupy
     * several slots after recycling — fire them as one group */
    std::map<uint64_t, std::vector<uint32_t>> fired;
    for (uint32_t s = 0; s < o->I; s++)
        if (tags[s] != EMPTY_TAG && tags[s] < wm) fired[tags[s]].push_back(s);
    for (auto &kv : fired)
        if (join_fire(o, kv.first, kv.second, c0, c1))
            return 1;
    if (out) {
        int64_t n = o->host_out.empty() ? 0 : (int64_t)o->host_out[0].size();
        if (op_out_alloc(o, out, n, o->out_cols, __func__)) return 1;
        for (int i = 0; n && i < o->out_cols; i++)
            memcpy(out->cols[i], o->host_out[i].data(), (size_t)n * 8);
        if (o->cfg.join_type != AMD_JOIN_INNER) {
            /* [key?, lvals, rvals, instant, lp, rp] */
            int base_l = o->cfg.n_keys;
            int inst = base_l + o->cfg.n_left_vals + o->cfg.n_right_vals;
            if (fill_join_validity(out, base_l, o->cfg.n_left_vals,
                                   o->cfg.n_right_vals, inst + 1, inst + 2)) {
                out_free_host(out);
                snprintf(o->err_msg, sizeof o->err_msg,
                         "validity bitmap allocation failed");
                return 1;
            }
        }
        for (auto &v : o->host_out) v.clear();
    }
    return 0;
}

/* drain one side's buffered rows: [key?, vals..., _timestamp] */
API int arroyo_amd_join_checkpoint_drain(void *h, int32_t side,
                                         AmdOutBatch *out) {
    GpuJoin *o = (GpuJoin *)h;
    if (op_check_err(o, join_err_msg)) return 1;
    int nv = side == 0 ? o->cfg.n_left_vals : o->cfg.n_right_vals;
    int ncols = o->cfg.n_keys + nv + 1;
    std::vector<uint64_t> tags(o->I);
    std::vector<unsigned long long> cur(o->I);
    HIP_CHECK(o, hipMemcpyAsync(tags.data(), o->tag, (size_t)o->I * 8,
                                hipMemcpyDeviceToHost, o->stream));
    HIP_CHECK(o, hipMemcpyAsync(cur.data(), o->cursor[side], (size_t)o->I * 8,
                                hipMemcpyDeviceToHost, o->stream));
    HIP_CHECK(o, hipStreamSynchronize(o->stream));
    int64_t total = 0;
    for (uint32_t s = 0; s < o->I; s++)
        if (tags[s] != EMPTY_TAG) total += (int64_t)cur[s];
    if (op_out_alloc(o, out, total, ncols, __func__)) return 1;
    size_t plane = (size_t)o->I * o->cap;
    int64_t r = 0;
    for (uint32_t s = 0; s < o->I; s++) {
        if (tags[s] == EMPTY_TAG || cur[s] == 0) continue;
        int64_t n = (int64_t)cur[s];
        int col = 0;
        if (o->cfg.n_keys) {
            HIP_CHECK(o, hipMemcpyAsync((int64_t *)out->cols[col] + r,
                                        o->key[side] + (size_t)s * o->cap,
                                        (size_t)n * 8, hipMemcpyDeviceToHost,
                                        o->stream));
            col++;
        }
        for (int v = 0; v < nv; v++, col++)
            HIP_CHECK(o, hipMemcpyAsync(
                    (int64_t *)out->cols[col] + r,
                    o->vals[side] + (size_t)v * plane + (size_t)s * o->cap,
                    (size_t)n * 8, hipMemcpyDeviceToHost, o->stream));
        HIP_CHECK(o, hipStreamSynchronize(o->stream));
        for (int64_t j = 0; j < n; j++)
            ((int64_t *)out->cols[ncols - 1])[r + j] = (int64_t)tags[s];
        r += n;
    }
    return 0;
}

API void arroyo_amd_join_destroy(void *h) {
    delete (GpuJoin *)h;   /* ~OpBase drains the stream first */
}
