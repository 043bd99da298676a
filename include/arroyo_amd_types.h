/* Shared POD types for the arroyo-amd C ABI.
 *
 * These mirror the configuration and batch contract of the reference's
 * windowed-aggregate operators (ArroyoSystems/arroyo):
 *   - AmdWindowConfig <-> api::SlidingWindowAggregateOperator /
 *     api::TumblingWindowAggregateOperator protobufs decoded at
 *     crates/arroyo-worker/src/arrow/sliding_aggregating_window.rs:449-528 and
 *     tumbling_aggregating_window.rs:111-201 (width/slide micros, input
 *     schema with key columns first, partial/final aggregation plans).  The
 *     serialized DataFusion plans are replaced by an explicit aggregate spec
 *     (op + input column), which is the information content of the plans for
 *     the supported aggregate set.
 *   - batch columns <-> Arrow RecordBatch per ArroyoSchema
 *     (crates/arroyo-rpc/src/df.rs:24-30: schema + timestamp_index +
 *     key_indices); key columns first, `_timestamp` (ns) last.
 *
 * Round-1 scope: fixed-width i64 key (0 or 1 key columns), i64 value
 * columns, non-nullable.  Timestamps are u64 nanoseconds since the epoch;
 * the end-of-stream watermark is UINT64_MAX (arroyo-worker watermark
 * generator on_close, watermark_generator.rs:131-148).
 */
#ifndef ARROYO_AMD_TYPES_H
#define ARROYO_AMD_TYPES_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum AmdAggOp {
    AMD_AGG_COUNT = 0, /* partial: count        final: sum of counts  */
    AMD_AGG_SUM   = 1, /* partial: sum (i64)    final: sum            */
    AMD_AGG_MIN   = 2, /* partial: min          final: min            */
    AMD_AGG_MAX   = 3, /* partial: max          final: max            */
    AMD_AGG_AVG   = 4, /* partial: (count,sum f64)  final: sum/divide */
    AMD_AGG_COUNT_DISTINCT = 5, /* updating aggregate only: exact count of
                                   distinct values under append+retract */
    /* round 2, updating aggregate only (every_aggregate.sql coverage):
     * retractable co-moment states.  n is the key's live row count (the
     * aggregated column is non-null unless the updating aggregate runs with
     * AmdUpdatingConfig.null_semantics = 1; then n is the count of live
     * rows whose argument is non-null), state = (sum(x) f64, sum(x^2) f64);
     * sample variants emit NaN when n < 2 (the reference emits SQL NULL
     * there, and so does null_semantics = 1, through the output validity
     * bitmap). */
    AMD_AGG_STDDEV = 6,
    AMD_AGG_STDDEV_POP = 7,
    AMD_AGG_VAR = 8,
    AMD_AGG_VAR_POP = 9,
    AMD_AGG_BIT_XOR = 10, /* xor is its own inverse: retract == append */
    /* two-argument co-moment family (updating aggregate only): state =
     * (sum y, sum x, sum xy, sum y^2, sum x^2) f64; the FIRST argument
     * (SQL's Y) is agg_col, the second (X) agg_col2.  Sample variants and
     * zero-variance cases emit NaN where the reference emits SQL NULL
     * (a NULL in the validity bitmap under null_semantics = 1, where a row
     * contributes only when both arguments are non-null). */
    AMD_AGG_COVAR_POP = 11,
    AMD_AGG_COVAR_SAMP = 12,
    AMD_AGG_CORR = 13,
    AMD_AGG_REGR_SLOPE = 14,
    AMD_AGG_REGR_INTERCEPT = 15,
    AMD_AGG_REGR_R2 = 16,
    AMD_AGG_REGR_AVGX = 17,
    AMD_AGG_REGR_AVGY = 18,
    AMD_AGG_REGR_COUNT = 19,   /* i64 output */
    AMD_AGG_REGR_SXX = 20,
    AMD_AGG_REGR_SYY = 21,
    AMD_AGG_REGR_SXY = 22,
    /* retractable bit aggregates: 64 per-bit u32 set-counts (32 state
     * words); AND = bit set in every live row, OR = in any.  bool_and /
     * bool_or are these over a 0/1 column. */
    AMD_AGG_BIT_AND = 23,
    AMD_AGG_BIT_OR = 24,
    /* order statistics under retraction (updating aggregate only; the
     * window, session and join operators reject them at create).  i64
     * input column, i64 output.  Each keeps the key's exact value multiset
     * (as COUNT DISTINCT does) and is selected from it at flush.
     * MEDIAN over the live multiset M of size W, sorted: odd W gives
     * M[W/2]; even W gives (M[(W-1)/2] + M[W/2]) / 2 in exact integer
     * arithmetic truncated toward zero, computed without 64-bit overflow
     * (DataFusion's integer median wherever its add does not wrap).
     * MIN_RETRACT / MAX_RETRACT are the retract-capable forms of MIN / MAX
     * a planner picks when the input is updating; AMD_AGG_MIN / MAX keep
     * their one-word append-only fast path. */
    AMD_AGG_MEDIAN = 25,
    AMD_AGG_MIN_RETRACT = 26,
    AMD_AGG_MAX_RETRACT = 27
};

#define AMD_MAX_AGGS 8

typedef struct {
    uint64_t width_nanos;
    uint64_t slide_nanos;     /* ignored when is_tumbling */
    int32_t  is_tumbling;     /* 1: TumblingAggregatingWindowFunc semantics */
    int32_t  n_keys;          /* 0 or 1 (i64 key columns, first) */
    int32_t  n_aggs;
    int32_t  agg_ops[AMD_MAX_AGGS];
    int32_t  agg_col[AMD_MAX_AGGS];  /* value-column index; -1 for COUNT(*) */
    int32_t  n_value_cols;    /* value columns between keys and _timestamp */
    uint32_t log2_capacity;   /* hash slots per pane (GPU path) */
    uint32_t ring_panes;      /* live-pane ring size (GPU path, power of 2) */
    int32_t  device;          /* HIP device ordinal (GPU path) */
    int32_t  emit_to_host;    /* GPU path: 1 = outputs copied to host memory */
    int32_t  val_is_f64[8];   /* value column v carries f64 bit patterns in
                                 its i64 plane (Arrow Float64 column);
                                 SUM/MIN/MAX/AVG over it aggregate as
                                 doubles and the output column is f64 */
} AmdWindowConfig;

/* Instant (windowed stream-stream) join configuration.  Mirrors
 * api::JoinOperator as decoded by InstantJoinConstructor
 * (crates/arroyo-worker/src/arrow/instant_join.rs:372-412): two keyed input
 * schemas and a join plan.  The serialized DataFusion HashJoinExec is
 * replaced by its information content for the supported shape: equi-join on
 * the (single i64) key column within each exact `_timestamp` instant
 * (rows are routed to per-instant execs, instant_join.rs:109-172; fired in
 * timestamp order when the watermark passes, :256-283).  n_keys=0 means the
 * join condition is the window/instant itself (e.g. windowed_inner_join.sql:
 * ON dropoffs.window = pickups.window) and each instant emits the cross
 * product of its sides.  Input batch columns per side: [key?, vals...,
 * _timestamp]; output: [key?, left vals..., right vals..., _timestamp].
 * join_type selects the reference's JoinType (planner plan/join.rs maps
 * LEFT/RIGHT/FULL onto the same per-instant HashJoinExec): non-inner
 * output gains two trailing presence columns [left_present, right_present]
 * (the C ABI's stand-in for Arrow validity bitmaps; absent side's value
 * columns are zero-filled).  Unmatched rows emit once, at instant fire. */
#define AMD_JOIN_INNER 0
#define AMD_JOIN_LEFT  1
#define AMD_JOIN_RIGHT 2
#define AMD_JOIN_FULL  3
typedef struct {
    int32_t  n_keys;            /* 0 or 1 */
    int32_t  n_left_vals;
    int32_t  n_right_vals;
    uint32_t log2_rows_cap;     /* per-instant per-side row capacity (GPU) */
    uint32_t instants;          /* live-instant slots (GPU, power of two) */
    uint32_t log2_out_cap;      /* output rows per fire (GPU) */
    int32_t  device;
    int32_t  emit_to_host;
    int32_t  join_type;         /* AMD_JOIN_* (default inner) */
} AmdJoinConfig;

/* Session (gap) window aggregate configuration.  Mirrors
 * api::SessionWindowAggregateOperator as decoded by
 * SessionAggregatingWindowConstructor
 * (crates/arroyo-worker/src/arrow/session_aggregating_window.rs:707-772):
 * gap_micros + input schema (keys first) + final aggregation plan.  The
 * serialized DataFusion plan is replaced by the explicit aggregate spec, as
 * for AmdWindowConfig.  Semantics (restated in oracle/arroyo_oracle.c and
 * arroyo_amd/csrc/session.hip): per key, rows sorted by time form maximal
 * runs where each next timestamp is strictly within (previous max + gap)
 * (ActiveSession::add_batch :424-495); a session fires when
 * data_end + gap < watermark (KeyComputingHolder::watermark_update
 * :559-608); output window = [min_ts, max_ts + gap), _timestamp = end - 1
 * (to_record_batch :316-380); rows with ts < watermark are dropped
 * (process_batch :849-874, gt_eq filter). */
typedef struct {
    int32_t  n_keys;            /* 0 or 1 */
    int32_t  n_value_cols;
    int32_t  n_aggs;
    int32_t  agg_ops[AMD_MAX_AGGS];  /* incl. AMD_AGG_COUNT_DISTINCT (one
                                        per op on the GPU path): exact
                                        per-session distinct count via
                                        single-writer hash regions */
    int32_t  agg_col[AMD_MAX_AGGS];
    uint64_t gap_nanos;
    uint32_t log2_capacity;     /* key slots in the session store (GPU) */
    uint32_t max_sessions;      /* live sessions held inline per key (GPU) */
    uint32_t log2_batch_capacity; /* per-batch pre-aggregation table (GPU) */
    uint32_t log2_out_cap;      /* output rows per watermark (GPU) */
    uint32_t log2_distinct;     /* per-session distinct-set capacity (GPU) */
    uint32_t log2_cd_regions;   /* distinct-set region pool (GPU) */
    int32_t  device;
    int32_t  emit_to_host;
} AmdSessionConfig;

/* Non-windowed (TTL'd) stream-stream join configuration.  Mirrors
 * api::JoinOperator as decoded by JoinWithExpirationConstructor
 * (crates/arroyo-worker/src/arrow/join_with_expiration.rs:213-267): two
 * keyed schemas + ttl_micros + join plan.  Semantics: each incoming batch
 * is inserted into its side's per-key state (KeyTimeView,
 * crates/arroyo-state/src/tables/expiring_time_key_map.rs:932-1050) and
 * immediately joined against the OTHER side's stored rows for its keys
 * (process_left/process_right :42-108) — inner equi-join on the i64 key,
 * output _timestamp = max(left._timestamp, right._timestamp)
 * (post_join_timestamp_projection,
 * crates/arroyo-planner/src/plan/join.rs:121-191).  The live in-memory view
 * never evicts during a run (TTL filters state only on restore,
 * table_manager.rs:533-570 passes the watermark to get_view); restore drops
 * rows with ts < watermark - ttl.
 *
 * join_type (AMD_JOIN_*) selects the reference's JoinType for updating
 * joins (the planner passes the SQL join type into the DataFusion join
 * inside JoinWithExpiration, plan/join.rs:326-379); non-inner output gains
 * trailing [left_present, right_present] columns (Arrow-validity stand-in)
 * and, because a later match must retract an earlier null-padded row, a
 * trailing is_retract column.  updating=1 means inputs carry retractions:
 * per-side layout becomes [key, vals..., is_retract, _timestamp], the
 * output gains the trailing is_retract column, and emissions maintain the
 * join incrementally (append/retract pairs as either side's multiset
 * changes).  CPU oracle only in round 1: the GPU library rejects
 * join_type != 0 or updating != 0 at create (no silent fallback). */
typedef struct {
    int32_t  n_keys;            /* 1 (i64 equi-join key) */
    int32_t  n_left_vals;
    int32_t  n_right_vals;
    uint64_t ttl_nanos;
    uint32_t log2_capacity;     /* key slots per side (GPU) */
    uint32_t log2_rows_cap;     /* stored-row pool per side (GPU) */
    uint32_t log2_out_cap;      /* output rows per process_batch (GPU) */
    int32_t  device;
    int32_t  emit_to_host;
    int32_t  join_type;         /* AMD_JOIN_* (default inner) */
    int32_t  updating;          /* 1 = inputs carry is_retract */
} AmdExpJoinConfig;

/* Updating (non-windowed) aggregate configuration.  Mirrors
 * api::UpdatingAggregateOperator as decoded by
 * IncrementalAggregatingFunc's constructor
 * (crates/arroyo-worker/src/arrow/incremental_aggregator.rs:1035-1193):
 * aggregate exprs + flush interval + ttl.  Semantics (restated in
 * oracle/arroyo_oracle.c and arroyo_amd/csrc/updagg.hip): per key,
 * retractable accumulators updated row by row (appends and, when the input
 * carries _updating_meta.is_retract, retractions); on flush
 * (handle_tick -> flush :637-737) every key touched since the last flush
 * emits retract(previously emitted value) + append(new value) -- the
 * retract omitted for first-time keys, the append omitted (retract only)
 * when the key's rows have all been retracted, and the whole pair skipped
 * when the value did not change.  COUNT/SUM/AVG retract by subtraction
 * (the reference's Sliding accumulators); COUNT DISTINCT keeps an exact
 * per-key value multiset (the reference's Batch accumulator,
 * IncrementalState::Batch :84-174); AMD_AGG_MIN / AMD_AGG_MAX are the
 * append-only one-word fast path (a retraction on them is a loud error);
 * AMD_AGG_MIN_RETRACT / AMD_AGG_MAX_RETRACT / AMD_AGG_MEDIAN keep the same
 * per-key value multiset as COUNT DISTINCT and re-select from it at flush,
 * which is what the reference's Batch accumulator does for min/max/median
 * over an updating input.  Their cost is linear in the distinct values a
 * key has ever held (log2_nodes bounds the pool; zero-net nodes are not
 * reclaimed).  Unknown op codes are rejected at create.  Flush cadence is
 * driven by the caller (the reference's tick timer).
 *
 * Float64 value columns (val_is_f64[c] = 1): column c travels as f64 bit
 * patterns in its i64 plane, on the host surface and on the *_device ones,
 * with and without null_semantics; a Float32 SQL column is widened to f64
 * by the caller.  The rules below are restated from DataFusion 48 and
 * arrow-arith, whose sources are not in the reference tree: restated, not
 * golden-pinned (the checker is the Python model tests/updagg_f64_ref.py;
 * the C oracle does not read the field).  For an aggregate whose argument
 * column is flagged: SUM keeps one f64 word starting at +0.0 (an append
 * adds v, a retraction adds -v) and AVG keeps (count, f64 sum); MIN / MAX /
 * MIN_RETRACT / MAX_RETRACT / MEDIAN order the values by IEEE totalOrder on
 * the bit patterns (-NaN < -inf < ... < -0.0 < +0.0 < ... < +inf < +NaN)
 * and return a stored value bit for bit, MEDIAN of an even count being
 * (lo + hi) / 2.0 as two IEEE binary64 operations (it may overflow to inf;
 * NaN propagates); the outputs of these are f64 and AmdOutBatch.is_f64 is
 * set.  The moment and co-moment families convert each argument by its own
 * column's flag (reinterpret when flagged, (double)v otherwise), so one
 * f64 and one i64 argument is legal; REGR_COUNT stays i64.  In an operator
 * with a flagged column every f64 sum word, those of AVG and the moments
 * over its i64 columns included, folds with the hardware f64 atomic add
 * (an operator without a flag keeps the compare-and-swap fold); both are
 * one IEEE add per row in arrival order.  flush and expire mark the same
 * output columns in AmdOutBatch.is_f64.  COUNT(col) is
 * unchanged.  COUNT DISTINCT is unchanged too: identity is by raw bits, so
 * -0.0 and +0.0 are two values and NaN payloads are distinct.  BIT_AND /
 * BIT_OR / BIT_XOR over a flagged column, a flag on a column index >=
 * n_value_cols and a flag value other than 0 / 1 are rejected at create.
 * f64 subtraction is not exact, so a key whose rows have all been retracted
 * could keep a residue in its sum words: the flush that finds a touched key
 * with zero live rows resets the sum words fed by a flagged column to +0.0
 * (the reference drops the key's accumulators there,
 * incremental_aggregator.rs:671-686), and expire clears the whole state.
 * Drain / restore carry state words raw: restoring into an operator with
 * different flags is the caller's error, as for every other config field.
 * val_is_f64 sits before null_semantics, which stays the struct's last
 * field: a caller compiled against the struct without val_is_f64 must be
 * rebuilt (its null_semantics would be read as val_is_f64[0]). */
typedef struct {
    int32_t  n_keys;            /* 0 or 1 */
    int32_t  n_value_cols;
    int32_t  n_aggs;
    int32_t  agg_col2[AMD_MAX_AGGS]; /* second argument (X) of the
                                        co-moment family; -1 otherwise */
    int32_t  agg_ops[AMD_MAX_AGGS];
    int32_t  agg_col[AMD_MAX_AGGS];
    uint32_t log2_capacity;     /* key slots (GPU) */
    uint32_t log2_nodes;        /* distinct-value node pool (GPU) */
    uint32_t log2_out_cap;
    int32_t  device;
    int32_t  emit_to_host;
    int32_t  val_is_f64[8];     /* per value column: 1 = the i64 plane holds
                                   f64 bit patterns (see above); all zeros is
                                   the i64 operator, bit for bit */
    int32_t  null_semantics;    /* 0: non-nullable value columns, NaN where
                                   the reference emits SQL NULL, no output
                                   validity (the contract above, unchanged).
                                   1: SQL NULL semantics -- value columns may
                                   carry Arrow validity bitmaps
                                   (updagg_process_batch_nullable), an
                                   aggregate skips rows whose argument is
                                   NULL (either argument for the co-moment
                                   family) and counts the remaining live
                                   rows n_a; COUNT / COUNT DISTINCT /
                                   REGR_COUNT are never NULL, every other
                                   aggregate is NULL when n_a == 0 or its
                                   result is undefined (sample variants at
                                   n_a < 2, zero-variance CORR / REGR_SLOPE
                                   / REGR_INTERCEPT / REGR_R2); flush and
                                   expire set AmdOutBatch.validity and the
                                   value under a NULL is 0 */
} AmdUpdatingConfig;

/* SQL window-function configuration.  Mirrors
 * api::WindowFunctionOperator as decoded by WindowFunctionConstructor
 * (crates/arroyo-worker/src/arrow/window_fn.rs:180-273): a
 * BoundedWindowAggExec run per exact `_timestamp` instant.  Semantics
 * (filter_and_split_batches :52-93, handle_watermark :220-246): rows are
 * buffered per instant (late rows ts < watermark silently filtered); when
 * the watermark passes an instant it fires in timestamp order, computing
 * fn(...) OVER (PARTITION BY part_col ORDER BY order cols <frame>) per row;
 * with a limit, rows whose function value is > limit are dropped (the
 * reference plans the downstream filter separately; fusing it here saves
 * materialising the full ranking).  Output columns: input columns +
 * trailing function value.
 *
 * The fields from `fn` on were appended: all zero they are ROW_NUMBER,
 * exactly the operator before them (the CPU oracle reads none of them and
 * numbers rows whatever they say).
 *
 * The functions (restated from DataFusion 48's window functions, whose
 * sources are not in the reference tree: NOT golden-pinned, the checker is
 * the independent restatement in tests/test_windowfn_funcs.py).  Rows sort
 * by partition, ORDER BY columns, arrival; peers are rows of one partition
 * equal on every ORDER BY column.  For the row at 0-based position t of a
 * partition of m rows, whose peer group spans positions ps..pe:
 *   ROW_NUMBER   t + 1
 *   RANK         ps + 1
 *   DENSE_RANK   peer groups up to and including its own
 *   LAG(arg, k)  arg at t - k if t - k >= 0, else default_value if
 *                has_default, else SQL NULL; k = 0 is the row's own value
 *   LEAD(arg, k) the same with t + k < m
 *   frame end e  t (ROWS), pe (RANGE), m - 1 (PARTITION); the frame always
 *                starts at position 0
 *   FIRST_VALUE  arg at 0            LAST_VALUE  arg at e
 *   SUM MIN MAX  over positions 0..e; SUM wraps in two's complement
 *   COUNT        e + 1
 * `arg` is a non-nullable i64 column.  NULLs (LAG/LEAD without a default)
 * leave through AmdOutBatch.validity of the function column, the value
 * under a NULL is 0; a batch without a NULL carries no validity table.
 * With limit == 0 a fired instant's rows come out in sort order
 * (partition, ORDER BY, arrival), instants in timestamp order.
 *
 * Rejected at create, each with its own message: an unknown fn or frame;
 * arg_col outside [0, n_cols - 2] for LAG LEAD FIRST_VALUE LAST_VALUE SUM
 * MIN MAX (COUNT also takes -1), arg_col != -1 for RANK and DENSE_RANK
 * (ROW_NUMBER takes -1 or the 0 of a zeroed tail); offset < 0; limit != 0
 * with anything but ROW_NUMBER RANK DENSE_RANK; frame != 0 for
 * ROW_NUMBER, the rank functions and LAG/LEAD, which ignore frames. */
enum {
    AMD_WFN_ROW_NUMBER = 0, AMD_WFN_RANK, AMD_WFN_DENSE_RANK, AMD_WFN_LAG,
    AMD_WFN_LEAD, AMD_WFN_FIRST_VALUE, AMD_WFN_LAST_VALUE, AMD_WFN_SUM,
    AMD_WFN_COUNT, AMD_WFN_MIN, AMD_WFN_MAX
};
enum {
    AMD_WFN_FRAME_RANGE = 0,      /* RANGE UNBOUNDED PRECEDING .. CURRENT ROW,
                                     peers included: DataFusion's default
                                     under an ORDER BY */
    AMD_WFN_FRAME_ROWS = 1,       /* ROWS UNBOUNDED PRECEDING .. CURRENT ROW */
    AMD_WFN_FRAME_PARTITION = 2   /* unbounded on both ends */
};
/* rows one block of the segmented-scan kernels covers per tile */
#define AMD_WFN_SCAN_TILE 2048

typedef struct {
    int32_t  n_cols;          /* input columns incl. trailing _timestamp */
    int32_t  part_col;        /* partition column index; -1 = whole instant */
    int32_t  n_order;         /* 1 or 2 ORDER BY columns */
    int32_t  order_col[2];
    int32_t  order_desc[2];
    int64_t  limit;           /* keep row_number <= limit; 0 = keep all */
    uint32_t log2_rows_cap;   /* per-instant row capacity (GPU) */
    uint32_t instants;        /* live-instant slots (GPU, power of two) */
    uint32_t log2_out_cap;
    int32_t  device;
    int32_t  emit_to_host;
    int32_t  fn;              /* AMD_WFN_*; 0 = ROW_NUMBER */
    int32_t  arg_col;         /* the function's value column; -1 = none */
    int32_t  frame;           /* AMD_WFN_FRAME_*; aggregates, FIRST_VALUE
                                 and LAST_VALUE only */
    int64_t  offset;          /* LAG/LEAD distance k >= 0, taken as it
                                 stands: 0 is the row's own value (SQL's
                                 default distance of 1 is supplied by
                                 whoever fills the config, as
                                 cabi.make_windowfn_config does) */
    int32_t  has_default;     /* LAG/LEAD: default_value instead of NULL */
    int64_t  default_value;
} AmdWindowFnConfig;

/* Stateless map/filter/projection configuration.  Replaces the reference's
 * expression operators (crates/arroyo-worker/src/arrow/mod.rs):
 * ValueExecutionOperator :48, ProjectionOperator :99, KeyExecutionOperator
 * :180 -- each runs a serialized DataFusion expression plan over every
 * batch.  Here the expression plan's information content is a small
 * register program evaluated per row: registers r0..r(n_in_cols-1) are
 * preloaded with the input columns, instructions write higher registers,
 * `out_reg` names the emitted columns (KeyExecutionOperator = key exprs
 * first), and `filter_reg` (when >= 0) keeps rows whose register is
 * nonzero, preserving row order like the reference's filter kernels.
 * i64 values and f64 bit patterns share the register file; AMD_MOP_I2F /
 * F2I convert.
 *
 * Arithmetic (restated from arrow-arith / DataFusion, pinned by
 * tests/test_mapop_ops.py):
 *   ADD SUB MUL   two's-complement wrapping
 *   DIV           truncates toward zero; b == 0 -> error "division by
 *                 zero"; INT64_MIN / -1 -> error "integer overflow ..."
 *   MOD           sign of the dividend; b == 0 -> "division by zero";
 *                 x % -1 == 0 for every x, INT64_MIN included
 *   EQ .. GE      signed 64-bit compare of the raw register (there are no
 *                 float compares); result exactly 0 or 1
 *   AND OR NOT    truthiness is != 0; result exactly 0 or 1
 *   I2F           round to nearest even
 *   F2I           truncates toward zero; NaN, +-inf or a value outside
 *                 [-2^63, 2^63) -> error "cast ... out of range"
 *   FADD .. FDIV  IEEE binary64, correctly rounded, subnormals kept
 *   filter        keeps a row iff the register is non-zero as an integer
 *                 (so the bit pattern of -0.0 is kept)
 * After a row error the call fails and returns no output; the next batch on
 * the handle is evaluated afresh.  If rows of one batch raise different
 * errors, which one is reported is unspecified.
 *
 * A config is validated at create (include/arroyo_amd_map_check.h): opcodes
 * and registers in range, and every register that is read -- by an
 * instruction, out_reg[] or filter_reg -- is an input register or the dst
 * of an earlier instruction.
 *
 * SQL NULLs (AmdMapConfig.null_semantics = 1; HIP operator only, the CPU
 * oracle rejects it at create).  Every register carries a validity bit next
 * to its value; input validity arrives as Arrow bitmaps through
 * arroyo_amd_map_process_batch_nullable[_device] and every output column
 * leaves with one.  Five more opcodes exist only in such a program (with
 * null_semantics = 0 they stay "unknown opcode"):
 *   IS_NULL      a          1 if a is NULL, else 0; never NULL
 *   IS_NOT_NULL  a          1 if a is valid, else 0; never NULL
 *   COALESCE     a, b       a if a is valid, else b (NULL if both are);
 *                           a raw 64-bit move
 *   NULLIF       a, b       NULL if a is NULL; a if b is NULL; NULL if the
 *                           raw i64 a == b; else a
 *   SELECT       a, b, imm  CASE WHEN a THEN b ELSE r[imm] END: b if a is
 *                           valid and nonzero, else register `imm`; value
 *                           and validity of the chosen branch.  `imm` is a
 *                           source register: 0 <= imm < AMD_MAP_MAX_REGS
 *                           and written earlier
 * The other opcodes under null_semantics = 1 (restated from arrow-arith /
 * DataFusion like the arithmetic above; NOT golden-pinned, the checker is
 * the independent reference in tests/test_mapop_null.py):
 *   ADD..MOD EQ..GE NOT I2F F2I FADD..FDIV
 *                NULL if any operand they read is NULL
 *   errors       a row whose result is NULL raises none: x / NULL, NULL / 0,
 *                NULL % 0 and F2I(NULL) are NULL (arrow-arith evaluates
 *                valid slots only); a valid x / 0 still errors
 *   AND          false if either side is valid-false, else NULL if either
 *                side is NULL, else true (Kleene)
 *   OR           true if either side is valid-true, else NULL if either
 *                side is NULL, else false (Kleene)
 *   CONST        always valid
 *   filter       keeps a row iff filter_reg is valid and nonzero: a NULL
 *                predicate drops the row
 *   values       the value under a NULL input is arbitrary and influences
 *                no result and no error; the value under a NULL output is
 *                exactly 0 (the updating aggregate's convention)
 * The machine is eager: both branches of a SELECT have already been
 * evaluated, errors included.  A guarded division therefore divides by a
 * NULLIF, never by the raw divisor:
 *   SELECT(b != 0, a / NULLIF(b, 0), else)
 * a / NULL is NULL and raises nothing, and SELECT then takes `else`. */
enum AmdMapOp {
    AMD_MOP_CONST = 0,  /* dst = imm */
    AMD_MOP_ADD, AMD_MOP_SUB, AMD_MOP_MUL, AMD_MOP_DIV, AMD_MOP_MOD,
    AMD_MOP_EQ, AMD_MOP_NE, AMD_MOP_LT, AMD_MOP_LE, AMD_MOP_GT, AMD_MOP_GE,
    AMD_MOP_AND, AMD_MOP_OR, AMD_MOP_NOT,
    AMD_MOP_I2F, AMD_MOP_F2I,    /* value <-> f64 bit pattern (truncating) */
    AMD_MOP_FADD, AMD_MOP_FSUB, AMD_MOP_FMUL, AMD_MOP_FDIV
};
/* opcodes 21..25, legal in null_semantics = 1 programs only (table above):
 * enum AmdMapNullOp */
#include "arroyo_amd_map_null.h"

#define AMD_MAP_MAX_PROG 64
#define AMD_MAP_MAX_REGS 32
#define AMD_MAP_MAX_OUT  16

typedef struct {
    int32_t op;     /* AmdMapOp */
    int32_t a, b;   /* source registers (b unused for unary/CONST) */
    int32_t dst;
    int64_t imm;    /* CONST value (f64 ops: bit pattern); SELECT: the
                       else-branch register */
} AmdMapInstr;

typedef struct {
    int32_t n_in_cols;          /* input columns incl. trailing _timestamp */
    int32_t n_prog;
    AmdMapInstr prog[AMD_MAP_MAX_PROG];
    int32_t n_out;
    int32_t out_reg[AMD_MAP_MAX_OUT];
    int32_t out_is_f64[AMD_MAP_MAX_OUT];
    int32_t filter_reg;         /* -1 = no filter */
    int32_t device;
    int32_t emit_to_host;
    int32_t null_semantics;     /* 0 = no NULLs (the contract above, byte for
                                   byte); 1 = SQL NULL semantics: a validity
                                   bit per register, opcodes 21..25 legal,
                                   bitmaps in and out */
} AmdMapConfig;

/* Output batch, allocated by the callee; free with *_free_out.
 * Column order: [key (if n_keys)], agg outputs (one column per agg),
 * window_start, window_end, _timestamp.  All columns are 8-byte elements;
 * is_f64[i] marks double columns (AVG outputs).  on_device=1 means `cols`
 * are HIP device pointers.
 *
 * validity: Arrow-layout per-column validity bitmaps (LSB order: bit
 * (r & 7) of byte (r >> 3) set = row r valid), or NULL when every column
 * is fully valid.  validity[c] == NULL marks column c all-valid.  The
 * outer-join operators set bitmaps on the null-padded value columns (the
 * Arrow RecordBatch contract of ArroyoSchema, crates/arroyo-rpc/src/
 * df.rs:24-30); the presence columns remain alongside for callers that
 * prefer flags. */
typedef struct {
    int64_t   n_rows;
    int32_t   n_cols;
    void    **cols;
    int32_t  *is_f64;
    int32_t   on_device;
    uint8_t **validity;
} AmdOutBatch;

/* Device string-key dictionary configuration (arroyo_amd_strkey_*).  The
 * reference keys its state maps on arbitrary Arrow types by row-encoding the
 * key tuple (crates/arroyo-state/src/tables/expiring_time_key_map.rs
 * :1008-1049); here an Arrow Utf8 key column is interned on device to stable
 * non-negative i64 ids that every operator above accepts as a key column.
 * At most 7/8 of the 1 << log2_capacity slots are used (half or less keeps
 * probes short); each interned string takes its length rounded up to 8 bytes
 * of the arena. */
typedef struct {
    int32_t device;
    int32_t log2_capacity;   /* hash slots = 1 << log2_capacity (1..30) */
    int64_t arena_bytes;     /* device byte arena for interned strings */
    int32_t hash_bits;       /* 0 = use the full 64-bit hash; k in 1..63 = keep
                              * only the low k bits of the hash for slot
                              * choice AND tag (forces collisions; exists so
                              * exactness-under-collision is testable) */
} AmdStrKeyConfig;

/* Strings out (decode and checkpoint drain), allocated by the callee in
 * host memory; free with arroyo_amd_strkey_free_out.  Arrow Utf8 layout. */
typedef struct {
    int64_t  n_rows;
    int64_t *ids;            /* [n_rows] (drain: the id of each string;
                              * decode: echo of the request) */
    int32_t *offsets;        /* [n_rows + 1], offsets[0] == 0 */
    uint8_t *data;           /* [offsets[n_rows]] */
} AmdStrBatch;

/* Device tuple-key dictionary configuration (arroyo_amd_tuplekey_*).  The
 * reference row-encodes the whole key tuple (expiring_time_key_map.rs
 * :1008-1049, as above): any number of columns, a SQL NULL being one more
 * key value.  Here a tuple of n_cols 64-bit words (i64, u64, f64 bit
 * patterns, strkey ids), each optionally NULL, is interned on device to a
 * stable non-negative i64 id that every operator above accepts as its
 * single key column.  At most 7/8 of the 1 << log2_capacity slots are used;
 * a slot takes 8 * (n_cols + 2) bytes of device memory. */
#define AMD_TKEY_MAX_COLS 8
/* the launch shape of the per-row kernels: blocks of AMD_TKEY_BLOCK_THREADS
 * threads, at most AMD_TKEY_MAX_BLOCKS of them, grid-stride over the rows.
 * Row counts around their product are edge cases of the kernels. */
#define AMD_TKEY_BLOCK_THREADS 256
#define AMD_TKEY_MAX_BLOCKS 2048

typedef struct {
    int32_t device;
    int32_t n_cols;          /* components per tuple, 1..AMD_TKEY_MAX_COLS */
    int32_t log2_capacity;   /* hash slots = 1 << log2_capacity (1..30) */
    int32_t hash_bits;       /* as AmdStrKeyConfig.hash_bits: 0 = the full
                              * 64-bit hash, k in 1..63 = only its low k bits
                              * for slot choice AND tag (forces collisions) */
    int32_t nullable;        /* 0: no validity bitmap is accepted or
                              * returned; 1: every component may carry an
                              * Arrow validity bitmap, in and out */
} AmdTupleKeyConfig;

/* Device keyed shuffle (arroyo_amd_shuffle_*): the stable partition ahead of
 * the cross-rank exchange (the reference's repartition, crates/
 * arroyo-operator/src/context.rs:506-560).  Every device buffer of a handle
 * is sized at create from max_rows / max_bytes; a call allocates nothing. */
#define AMD_SHUF_KEY_I64  0  /* owner = hash64(cols[key_col]) / range, the
                              * splitmix64 + range rule of arroyo_amd_partition */
#define AMD_SHUF_KEY_HASH 1  /* cols[key_col] already is a 64-bit hash (the
                              * strkey content hash), used as is */
#define AMD_SHUF_MAX_COLS 16
#define AMD_SHUF_MAX_PARTS 64
#define AMD_SHUF_MAX_ROWS (1LL << 30)
#define AMD_SHUF_N_KERNELS 5 /* count, scan, scatter, utf8 offsets, utf8 copy */
#define AMD_SHUF_TILE_ROWS 1024 /* consecutive rows one block counts and
                                 * scatters; sizes around it are the edge
                                 * cases of the kernels */

typedef struct {
    int32_t device;
    int32_t n_parts;         /* 1..AMD_SHUF_MAX_PARTS */
    int32_t n_cols;          /* 8-byte columns carried (i64, u64 or f64 bit
                              * patterns), 1..AMD_SHUF_MAX_COLS, the key
                              * column among them */
    int32_t key_col;         /* 0..n_cols - 1 */
    int32_t key_mode;        /* AMD_SHUF_KEY_* */
    int32_t has_utf8;        /* 1: one Arrow Utf8 column rides along */
    int64_t max_rows;        /* rows per call, 1..AMD_SHUF_MAX_ROWS */
    int64_t max_bytes;       /* Utf8 bytes per call, 0..INT32_MAX */
} AmdShuffleConfig;

/* Result of one partition call.  The pointers are device memory owned by the
 * handle, valid until the next call on it; the starts are host values.
 * Partition p is rows [row_start[p], row_start[p + 1]) of every column, in
 * input order.  Its strings are a standalone Arrow Utf8 array: the
 * row_start[p + 1] - row_start[p] + 1 offsets from index row_start[p] + p of
 * utf8_offsets (the first is 0), relative to utf8_data + byte_start[p]; its
 * bytes are [byte_start[p], byte_start[p + 1]). */
typedef struct {
    int64_t  n_rows;
    int64_t *cols[AMD_SHUF_MAX_COLS];
    int32_t *utf8_offsets;   /* n_rows + n_parts entries */
    uint8_t *utf8_data;
    int64_t  row_start[AMD_SHUF_MAX_PARTS + 1];
    int64_t  byte_start[AMD_SHUF_MAX_PARTS + 1];
} AmdShuffleOut;

#ifdef __cplusplus
}
#endif

#endif /* ARROYO_AMD_TYPES_H */
