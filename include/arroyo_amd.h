/* arroyo-amd C ABI: the drop-in boundary for the MI355X-native execution
 * path of Arroyo's windowed-aggregate operators.
 *
 * Each entry point replaces one method of the reference's `ArrowOperator`
 * trait (ArroyoSystems/arroyo, crates/arroyo-operator/src/operator.rs), with
 * the same ownership and threading contract: one thread of execution per
 * handle, operator receives owned immutable batches, emits owned batches.
 * The Rust host would bind these over FFI (see INTEGRATION.md for the
 * ready-to-paste binding) exactly where OperatorConstructor::with_config and
 * the operator methods are invoked today:
 *
 *   arroyo_amd_create           <-> OperatorConstructor::with_config
 *                                   (operator.rs:56-63; config contents from
 *                                   api::SlidingWindowAggregateOperator,
 *                                   sliding_aggregating_window.rs:449-528)
 *   arroyo_amd_process_batch    <-> ArrowOperator::process_batch
 *                                   (operator.rs:1183;
 *                                   sliding_aggregating_window.rs:598-674)
 *   arroyo_amd_handle_watermark <-> ArrowOperator::handle_watermark
 *                                   (operator.rs:1208; sliding :676-691);
 *                                   emitted batches = Collector::collect
 *                                   calls (context.rs:491-494)
 *   arroyo_amd_checkpoint_drain <-> ArrowOperator::handle_checkpoint
 *                                   (operator.rs:1218; sliding :693-737)
 *   arroyo_amd_restore          <-> ArrowOperator::on_start restore
 *                                   (operator.rs:1167; sliding :556-595)
 *   arroyo_amd_destroy          <-> operator drop
 *   arroyo_amd_partition        <-> ArrowCollector::repartition +
 *                                   server_for_hash_array
 *                                   (context.rs:506-560,
 *                                   arroyo-operator/src/lib.rs:30-41) --
 *                                   device-side partitioning for the keyed
 *                                   shuffle; the exchange itself is RCCL
 *                                   all-to-all over xGMI at harness level.
 *
 * Batches are Arrow-layout columns (8-byte fixed-width values buffers, key
 * columns first, `_timestamp` in nanoseconds last -- ArroyoSchema,
 * arroyo-rpc/src/df.rs:24-30).  Timestamps/watermarks are u64 ns since the
 * epoch; the end-of-stream watermark is UINT64_MAX.  Errors: non-zero return
 * + arroyo_amd_last_error(handle).
 */
#ifndef ARROYO_AMD_H
#define ARROYO_AMD_H

#include "arroyo_amd_types.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Create a sliding/tumbling window-aggregate operator on cfg->device.
 * Returns NULL on failure (message via arroyo_amd_last_error(NULL)).
 * Requires a HIP device: there is no CPU fallback. */
void *arroyo_amd_create(const AmdWindowConfig *cfg);

/* Ingest one batch of host-memory columns
 * [keys..., values..., _timestamp], each `n_rows` i64 values. */
int arroyo_amd_process_batch(void *h, const int64_t *const *cols,
                             int32_t n_cols, int64_t n_rows);

/* Same, with columns already resident in device HBM; ts_offset is added to
 * every timestamp (synthetic-stream ring replay). */
int arroyo_amd_process_batch_device(void *h, const int64_t *const *dcols,
                                    int32_t n_cols, int64_t n_rows,
                                    uint64_t ts_offset);

/* Submit `reps` device-resident batches in one call (one kernel launch per
 * batch).  contiguous=1: batch k = rows [k*n_rows,(k+1)*n_rows) of dcols;
 * contiguous=0: the same rows replayed.  ts_offset advances by ts_step per
 * batch.  Keeps per-batch FFI overhead off the hot loop. */
int arroyo_amd_process_batches_device(void *h, const int64_t *const *dcols,
                                      int32_t n_cols, int64_t n_rows,
                                      int32_t reps, int32_t contiguous,
                                      uint64_t ts_offset0, uint64_t ts_step);

/* Streaming-read bandwidth calibration over two n-row i64 device columns;
 * returns GB/s (measurement tooling). */
double arroyo_amd_stream_gbps(const void *d_a, const void *d_b, int64_t n,
                              int iters);

/* Synchronize the operator's internal stream: callers that reuse
 * device buffers handed to process_batch_device (e.g. the N>1 bench's
 * RCCL exchange buffers) must fence the consuming kernels first. */
int arroyo_amd_sync(void *h);

/* Advance the watermark; fires every window the reference would fire, in
 * order, and returns the emitted rows (all fired windows concatenated;
 * column order [key?, aggs..., window_start, window_end, _timestamp]).
 * `out` may be NULL to defer collection to a later call. */
int arroyo_amd_handle_watermark(void *h, uint64_t watermark_nanos,
                                AmdOutBatch *out);

/* Batched form of handle_watermark for a group of watermarks with NO
 * process_batch between them (the periodic WatermarkGenerator emits such
 * runs whenever the source idles; the bench's fused periods do too).
 * Equivalent to calling handle_watermark(wms[i]) in order, but the
 * device status (pane tags, min non-late bin) is read ONCE for the whole
 * group — each per-watermark read costs a stream sync (~15 us idle). */
int arroyo_amd_handle_watermarks(void *h, const uint64_t *wms, int32_t n,
                                 AmdOutBatch *out);

/* Epoch pipelining: lets a harness submit the NEXT period's batches
 * before folding this period's watermarks, hiding the fold's host
 * latency behind the next period's kernels.  Sequence:
 *   submit(g); mark_epoch(); set_filter_watermark(last wm of group g);
 *   submit(g+1); handle_watermarks_epoch(group g's wms, out);
 * mark_epoch snapshots the device status at period g's stream point
 * (depth 2).  set_filter_watermark pre-advances the ingest late-drop
 * cutoff to the watermark the deferred group will establish, so the
 * next period's rows are filtered exactly as in the sequential order;
 * emissions are bit-identical to sequential handle_watermark calls. */
int arroyo_amd_set_filter_watermark(void *h, uint64_t watermark_nanos);
int arroyo_amd_mark_epoch(void *h);
int arroyo_amd_handle_watermarks_epoch(void *h, const uint64_t *wms,
                                       int32_t n, AmdOutBatch *out);

/* Drain open panes' partial states for a checkpoint barrier.  Columns:
 * [key?, partial state words (AVG takes 2)..., bin _timestamp]. */
int arroyo_amd_checkpoint_drain(void *h, AmdOutBatch *out);

/* Restore checkpointed partial states (layout as checkpoint_drain). */
int arroyo_amd_restore(void *h, const int64_t *const *cols, int32_t n_cols,
                       int64_t n_rows, int has_watermark,
                       uint64_t watermark_nanos);

void arroyo_amd_free_out(AmdOutBatch *out);
void arroyo_amd_destroy(void *h);
const char *arroyo_amd_last_error(void *h);

/* Dominant-kernel timing for the measurement harness: total update-kernel
 * time (HIP events on the operator's stream), rows processed, launches, and rows
 * emitted device-side since the last call. */
int arroyo_amd_perf(void *h, double *update_ms, int64_t *rows,
                    int64_t *launches, int64_t *emitted_device_rows);

/* Output introspection for the measurement harness: host copy of the window
 * emissions still resident in the device output buffers (the latest fired
 * window per fire stream; row order within a window is unspecified).  Free
 * with arroyo_amd_free_out. */
int arroyo_amd_last_emission(void *h, AmdOutBatch *out);

/* Device-side key-hash partitioning (shuffle): writes rows regrouped into
 * per-partition contiguous segments and per-partition counts. */
int arroyo_amd_partition(const int64_t *d_keys, const int64_t *d_vals,
                         const int64_t *d_ts, int64_t n, uint32_t n_parts,
                         int64_t *d_out_keys, int64_t *d_out_vals,
                         int64_t *d_out_ts, uint64_t *h_counts);

/* ---- instant (windowed stream-stream) join ----------------------------
 * Replaces InstantJoin (crates/arroyo-worker/src/arrow/instant_join.rs)
 * behind the same ArrowOperator surface:
 *   join_create          <-> InstantJoinConstructor::with_config (:372-412)
 *   join_process_batch   <-> process_batch_index left/right routing
 *                            (:241-255 -> process_side :109-172); side 0 =
 *                            left, 1 = right; cols [key?, vals, _timestamp]
 *   join_handle_watermark<-> handle_watermark (:256-283): fires every
 *                            instant < wm in timestamp order; out columns
 *                            [key?, left vals..., right vals..., _timestamp]
 *   join_checkpoint_drain<-> handle_checkpoint (:285-303): one side's
 *                            buffered rows
 *   join_restore          = process_batch (on_start re-processes the
 *                            drained batches, :205-230)                  */
void *arroyo_amd_join_create(const AmdJoinConfig *cfg);
int arroyo_amd_join_process_batch(void *h, int32_t side,
                                  const int64_t *const *cols, int32_t n_cols,
                                  int64_t n_rows);
int arroyo_amd_join_process_batch_device(void *h, int32_t side,
                                         const int64_t *const *dcols,
                                         int32_t n_cols, int64_t n_rows);
int arroyo_amd_join_handle_watermark(void *h, uint64_t watermark_nanos,
                                     AmdOutBatch *out);
int arroyo_amd_join_checkpoint_drain(void *h, int32_t side, AmdOutBatch *out);
void arroyo_amd_join_destroy(void *h);
const char *arroyo_amd_join_last_error(void *h);

/* ---- session (gap) window aggregate -----------------------------------
 * Replaces SessionAggregatingWindowFunc
 * (crates/arroyo-worker/src/arrow/session_aggregating_window.rs) behind the
 * same ArrowOperator surface:
 *   session_create           <-> SessionAggregatingWindowConstructor
 *                                ::with_config (:707-772)
 *   session_process_batch    <-> process_batch (:849-893): late rows
 *                                (ts < watermark) silently dropped, rest
 *                                buffered into per-key session state
 *   session_handle_watermark <-> handle_watermark -> advance (:76-98,
 *                                :894-903): fires every session with
 *                                data_end + gap < watermark; out columns
 *                                [key?, aggs..., window_start, window_end,
 *                                _timestamp = window_end - 1]
 *   session_checkpoint_drain <-> handle_checkpoint (:905-921): live session
 *                                partial states [key?, state words...,
 *                                data_start, data_end]
 *   session_restore          <-> on_start (:803-846): reload drained
 *                                partial sessions
 */
void *arroyo_amd_session_create(const AmdSessionConfig *cfg);
int arroyo_amd_session_process_batch(void *h, const int64_t *const *cols,
                                     int32_t n_cols, int64_t n_rows);
int arroyo_amd_session_process_batch_device(void *h,
                                            const int64_t *const *dcols,
                                            int32_t n_cols, int64_t n_rows,
                                            uint64_t ts_offset);
int arroyo_amd_session_handle_watermark(void *h, uint64_t watermark_nanos,
                                        AmdOutBatch *out);
int arroyo_amd_session_checkpoint_drain(void *h, AmdOutBatch *out);
/* COUNT DISTINCT value stream for checkpoints: one row per live
 * (session, value): [key?, session_start, value]; restore after
 * session_restore (which zeroes the CD words it rebuilds) */
int arroyo_amd_session_drain_values(void *h, AmdOutBatch *out);
int arroyo_amd_session_restore_values(void *h, const int64_t *const *cols,
                                      int32_t n_cols, int64_t n_rows);
int arroyo_amd_session_restore(void *h, const int64_t *const *cols,
                               int32_t n_cols, int64_t n_rows);
void arroyo_amd_session_destroy(void *h);
const char *arroyo_amd_session_last_error(void *h);

/* ---- non-windowed (TTL'd) stream-stream join --------------------------
 * Replaces JoinWithExpiration
 * (crates/arroyo-worker/src/arrow/join_with_expiration.rs) behind the same
 * ArrowOperator surface:
 *   expjoin_create          <-> JoinWithExpirationConstructor::with_config
 *                               (:213-267)
 *   expjoin_process_batch   <-> process_batch_index (:162-180) ->
 *                               process_left/process_right (:42-108):
 *                               inserts the batch into its side's per-key
 *                               state AND returns the joined output rows
 *                               [key, left vals..., right vals...,
 *                               _timestamp = max(l_ts, r_ts)] against the
 *                               other side's stored rows
 *   expjoin_handle_watermark:   records the watermark (live state never
 *                               evicts during a run, table_manager.rs:533;
 *                               TTL applies on restore)
 *   expjoin_expire          :   explicit eviction of rows with
 *                               ts < watermark - ttl (bounded-memory mode;
 *                               matches what the reference's state layer
 *                               drops across checkpoint/restore)
 *   expjoin_checkpoint_drain<-> tables() flush: one side's stored rows
 *   expjoin_restore         <-> on_start: reload rows, dropping those with
 *                               ts < watermark - ttl (get_key_time_table
 *                               restore filter)
 */
void *arroyo_amd_expjoin_create(const AmdExpJoinConfig *cfg);
int arroyo_amd_expjoin_process_batch(void *h, int32_t side,
                                     const int64_t *const *cols,
                                     int32_t n_cols, int64_t n_rows,
                                     AmdOutBatch *out);
int arroyo_amd_expjoin_process_batch_device(void *h, int32_t side,
                                            const int64_t *const *dcols,
                                            int32_t n_cols, int64_t n_rows);
int arroyo_amd_expjoin_collect(void *h, AmdOutBatch *out);
int arroyo_amd_expjoin_handle_watermark(void *h, uint64_t watermark_nanos);

/* Device-resident consumption: report and reset the accumulated match
 * count without host copies (the next stage consumes the device match
 * columns in place). */
int arroyo_amd_expjoin_match_count(void *h, int64_t *n_matches);
int arroyo_amd_expjoin_expire(void *h);
int arroyo_amd_expjoin_checkpoint_drain(void *h, int32_t side,
                                        AmdOutBatch *out);
int arroyo_amd_expjoin_restore(void *h, int32_t side,
                               const int64_t *const *cols, int32_t n_cols,
                               int64_t n_rows, int has_watermark,
                               uint64_t watermark_nanos);
void arroyo_amd_expjoin_destroy(void *h);
const char *arroyo_amd_expjoin_last_error(void *h);

/* ---- updating (non-windowed) aggregate --------------------------------
 * Replaces IncrementalAggregatingFunc
 * (crates/arroyo-worker/src/arrow/incremental_aggregator.rs) behind the
 * same ArrowOperator surface:
 *   updagg_create        <-> constructor (:1035-1193)
 *   updagg_process_batch <-> process_batch (:931-949) ->
 *                            keyed_aggregate/global_aggregate (:778-884);
 *                            cols [key?, vals..., is_retract] where
 *                            is_retract mirrors _updating_meta.is_retract
 *                            (get_retracts :740-758); a value column
 *                            flagged in cfg.val_is_f64 holds f64 bit
 *                            patterns, on every ingest surface
 *   updagg_flush         <-> handle_tick/on_close -> flush (:637-737):
 *                            out columns [key?, agg outputs...,
 *                            is_retract]
 *   updagg_checkpoint_drain(which): which=0 scalar accumulator states
 *                            (the "a" table, checkpoint_sliding :271-340),
 *                            which=1 distinct-value multiset rows
 *                            [key?, agg_index, value, net_count] (the "b"
 *                            table, checkpoint_batch :342-418)
 *   updagg_restore       <-> on_start -> initialize (:446-599)
 */
void *arroyo_amd_updagg_create(const AmdUpdatingConfig *cfg);
int arroyo_amd_updagg_process_batch(void *h, const int64_t *const *cols,
                                    int32_t n_cols, int64_t n_rows);
int arroyo_amd_updagg_process_batch_device(void *h,
                                           const int64_t *const *dcols,
                                           int32_t n_cols, int64_t n_rows);
/* Nullable ingest (handles created with null_semantics = 1 only; a loud
 * error otherwise).  `validity` may be NULL (everything valid) and
 * validity[c] may be NULL (column c all valid); otherwise validity[c] is an
 * Arrow validity bitmap -- LSB bit order, bit offset 0, (n_rows + 7) / 8
 * bytes, the layout of AmdOutBatch.validity.  A bitmap on the key column or
 * on is_retract is an error (NULL group keys are not supported).  The host
 * surface stages the data and makes no alignment or padding demand.  The
 * device surface reads the bitmaps in place as 64-bit words: each
 * dvalidity[c] must be 8-byte aligned and its buffer padded to a multiple
 * of 8 bytes (Arrow buffers are).  The plain process_batch* calls stay
 * legal on a null_semantics = 1 handle and mean "all valid".  Under
 * null_semantics = 1, flush and expire set out->validity: NULL pointers for
 * the key and is_retract columns and for an aggregate column whose emitted
 * rows are all valid, a bitmap otherwise (freed by arroyo_amd_free_out);
 * checkpoint_drain(0) rows gain one trailing column, the validity mask of
 * the key's last emitted row (bit a = aggregate a non-NULL). */
int arroyo_amd_updagg_process_batch_nullable(void *h,
                                             const int64_t *const *cols,
                                             const uint8_t *const *validity,
                                             int32_t n_cols, int64_t n_rows);
int arroyo_amd_updagg_process_batch_nullable_device(
    void *h, const int64_t *const *dcols, const uint8_t *const *dvalidity,
    int32_t n_cols, int64_t n_rows);
int arroyo_amd_updagg_flush(void *h, AmdOutBatch *out);
/* TTL eviction of keys idle for more than `idle_flushes` flush epochs
 * (the reference's UpdatingCache::time_out, wall-clock there); emits the
 * retract rows */
int arroyo_amd_updagg_expire(void *h, int64_t idle_flushes, AmdOutBatch *out);
int arroyo_amd_updagg_checkpoint_drain(void *h, int32_t which,
                                       AmdOutBatch *out);
int arroyo_amd_updagg_restore(void *h, int32_t which,
                              const int64_t *const *cols, int32_t n_cols,
                              int64_t n_rows);
void arroyo_amd_updagg_destroy(void *h);
const char *arroyo_amd_updagg_last_error(void *h);

/* ---- SQL window functions (per instant) -------------------------------
 * Replaces WindowFunctionOperator
 * (crates/arroyo-worker/src/arrow/window_fn.rs) behind the same
 * ArrowOperator surface:
 *   windowfn_create           <-> WindowFunctionConstructor (:180-273);
 *                                 AmdWindowFnConfig.fn picks the function
 *                                 (AMD_WFN_*: ROW_NUMBER, RANK, DENSE_RANK,
 *                                 LAG, LEAD, FIRST_VALUE, LAST_VALUE, SUM,
 *                                 COUNT, MIN, MAX), .frame its frame; the
 *                                 CPU oracle implements ROW_NUMBER only
 *   windowfn_process_batch    <-> process_batch (:275-300): buffers rows
 *                                 per exact instant; late rows silently
 *                                 filtered (filter_and_split_batches)
 *   windowfn_handle_watermark <-> handle_watermark (:220-246): fires
 *                                 instants < wm in timestamp order; out
 *                                 columns [input cols..., function value];
 *                                 LAG/LEAD without a default set
 *                                 out->validity of the function column
 *                                 where a NULL occurs
 *   windowfn_checkpoint_drain <-> handle_checkpoint (:302-324): buffered
 *                                 rows in arrival order; restore =
 *                                 process_batch
 */
void *arroyo_amd_windowfn_create(const AmdWindowFnConfig *cfg);
int arroyo_amd_windowfn_process_batch(void *h, const int64_t *const *cols,
                                      int32_t n_cols, int64_t n_rows);
int arroyo_amd_windowfn_process_batch_device(void *h,
                                             const int64_t *const *dcols,
                                             int32_t n_cols, int64_t n_rows);
int arroyo_amd_windowfn_restore(void *h, const int64_t *const *cols,
                                int32_t n_cols, int64_t n_rows);
int arroyo_amd_windowfn_handle_watermark(void *h, uint64_t watermark_nanos,
                                         AmdOutBatch *out);
int arroyo_amd_windowfn_checkpoint_drain(void *h, AmdOutBatch *out);
void arroyo_amd_windowfn_destroy(void *h);
const char *arroyo_amd_windowfn_last_error(void *h);

/* ---- stateless map / filter / projection ------------------------------
 * Replaces ValueExecutionOperator / ProjectionOperator /
 * KeyExecutionOperator (crates/arroyo-worker/src/arrow/mod.rs:48-243):
 *   map_create        <-> the operators' constructors (:70-97, :127-178,
 *                         :213-243): the serialized expression plan becomes
 *                         the register program in AmdMapConfig
 *   map_process_batch <-> process_batch (:56-68, :112-125, :196-211):
 *                         stateless, emits the projected (and filtered,
 *                         order-preserving) rows immediately
 * No state: nothing to checkpoint (the reference's tables() are empty). */
void *arroyo_amd_map_create(const AmdMapConfig *cfg);
int arroyo_amd_map_process_batch(void *h, const int64_t *const *cols,
                                 int32_t n_cols, int64_t n_rows,
                                 AmdOutBatch *out);
int arroyo_amd_map_process_batch_device(void *h, const int64_t *const *dcols,
                                        int32_t n_cols, int64_t n_rows,
                                        const int64_t **d_out_cols,
                                        int64_t *n_out_rows);
/* SQL NULLs through the map (AmdMapConfig.null_semantics = 1; opcode table,
 * propagation rules and the NULLIF idiom for a guarded division are in
 * arroyo_amd_types.h).  These sit between the outer joins, which emit
 * validity bitmaps, and the nullable updating aggregate, which takes them.
 *
 * Bitmaps are Arrow's: LSB first, bit offset 0, (n_rows + 7) / 8 bytes.
 * `validity` may be NULL and validity[c] may be NULL: all valid.  Any
 * column, _timestamp included, may carry one; padding bits past n_rows may
 * hold anything.
 *   host surface    no alignment or padding demand on the input; chunks at
 *                   the operator's capacity.  out->validity[c] is NULL for
 *                   a column whose emitted rows are all valid and
 *                   out->validity itself when every column is; padding bits
 *                   are clear; the value under a NULL is 0
 *   device surface  each dvalidity[c] is 8-byte aligned and padded to a
 *                   multiple of 8 bytes (read in place as 64-bit words);
 *                   n_rows above the capacity is an error.  Every
 *                   d_out_validity[i] is a device bitmap owned by the
 *                   operator until the next call, 8-byte aligned, padded to
 *                   8 bytes, padding bits clear; null_counts[i] (host) is
 *                   the number of NULLs in emitted column i, so a
 *                   downstream call may pass NULL for a column with 0
 * The nullable calls on a null_semantics = 0 handle fail.  On a
 * null_semantics = 1 handle the plain map_process_batch is legal -- every
 * input valid -- and still fills out->validity, as NULLIF and COALESCE make
 * NULLs of their own; the plain map_process_batch_device fails, having no
 * way to return bitmaps. */
int arroyo_amd_map_process_batch_nullable(void *h,
                                          const int64_t *const *cols,
                                          const uint8_t *const *validity,
                                          int32_t n_cols, int64_t n_rows,
                                          AmdOutBatch *out);
int arroyo_amd_map_process_batch_nullable_device(
    void *h, const int64_t *const *dcols, const uint8_t *const *dvalidity,
    int32_t n_cols, int64_t n_rows, const int64_t **d_out_cols,
    const uint8_t **d_out_validity, int64_t *null_counts,
    int64_t *n_out_rows);
void arroyo_amd_map_destroy(void *h);
const char *arroyo_amd_map_last_error(void *h);

/* ---- device string-key dictionary --------------------------------------
 * The reference keys state on arbitrary Arrow types by row-encoding the key
 * tuple (crates/arroyo-state/src/tables/expiring_time_key_map.rs:1008-1049);
 * SQL such as `GROUP BY event_type` keys on Utf8.  This family interns an
 * Arrow Utf8 array (int32 offsets + byte buffer) on device: every string
 * maps to an opaque, stable, non-negative i64 id that any operator above
 * accepts as a key column, and ids map back to strings at emission.  It has
 * no window or watermark logic; it sits in front of and behind the other
 * operators.  One handle is shared by every operator that must agree on the
 * ids: both sides of a join keyed on the same column, or a map -> window ->
 * window-function chain.
 *
 *   strkey_encode / _device   <-> the key row-encoding ahead of process_batch
 *   strkey_decode             <-> rebuilding the key column of an emission
 *   strkey_checkpoint_drain / strkey_restore
 *                             <-> part of the keyed operators' checkpoint:
 *                                 their drained state refers to these ids
 *
 * Offsets: n_rows + 1 entries; row r is data[offsets[r] .. offsets[r+1]);
 * offsets[0] may be non-zero (a sliced array).  No byte of `data` outside
 * [offsets[0], offsets[n_rows]) is ever read.  A negative or decreasing
 * offset is an error, detected on the device before any byte is read.
 *
 * Ids: equal byte strings get equal ids and different byte strings get
 * different ids, for the life of the handle and across batches; only a full
 * length-and-bytes compare decides identity.  The empty string, embedded NUL
 * bytes and non-UTF-8 bytes are legal.  Ids are opaque; callers may assume
 * only id >= 0 (never the engines' EMPTY_KEY).
 *
 * Hashes: hashes_out / d_hashes_out may be NULL; otherwise they receive a
 * 64-bit content hash per row, a pure function of the bytes, identical
 * across handles, devices and hash_bits.  Ids are per handle, so a keyed
 * shuffle must partition on this hash, never on the ids.
 *
 * The device surface takes device pointers, runs on the handle's own stream
 * and synchronises before returning, so a chained *_process_batch_device on
 * another handle may consume d_ids_out directly.
 *
 * decode gathers on the device and returns malloc'd host buffers; an id that
 * was never issued, or a total above INT32_MAX bytes, is an error.  A full
 * dictionary ("capacity") or arena ("arena") is an error; strings interned
 * by earlier calls stay valid, ids_out of the failing call are undefined.
 *
 * checkpoint_drain returns every interned string with its id; restore loads
 * that into an EMPTY handle (anything else is an error) so every string
 * keeps its id.  An id is a slot of the hash table, so the restoring handle
 * needs the same log2_capacity and hash_bits; a mismatch is an error and
 * leaves the handle empty.
 *
 * Out of scope: LargeUtf8 (int64 offsets); NULL keys here (no validity
 * bitmap is accepted: a nullable string key goes through the tuple-key
 * dictionary below, its strkey id as the component and its validity bitmap
 * alongside); eviction (ids must stay stable for
 * live state, as for the composite-key dictionary); the oracle has no
 * counterpart -- a host dictionary is the checker for an interner. */
void *arroyo_amd_strkey_create(const AmdStrKeyConfig *cfg);
int arroyo_amd_strkey_encode(void *h, const int32_t *offsets,
                             const uint8_t *data, int64_t n_rows,
                             int64_t *ids_out, uint64_t *hashes_out);
int arroyo_amd_strkey_encode_device(void *h, const int32_t *d_offsets,
                                    const uint8_t *d_data, int64_t n_rows,
                                    int64_t *d_ids_out,
                                    uint64_t *d_hashes_out);
int arroyo_amd_strkey_decode(void *h, const int64_t *ids, int64_t n_rows,
                             AmdStrBatch *out);
int arroyo_amd_strkey_count(void *h, int64_t *n_strings, int64_t *arena_used);
int arroyo_amd_strkey_checkpoint_drain(void *h, AmdStrBatch *out);
int arroyo_amd_strkey_restore(void *h, const int64_t *ids,
                              const int32_t *offsets, const uint8_t *data,
                              int64_t n_rows);
/* Measurement aid: enable > 0 makes every later encode time its lookup
 * (probe) kernel alone with HIP events, enable == 0 stops that, enable < 0
 * leaves the setting; *last_lookup_ms (may be NULL) receives the kernel time
 * of the last timed encode. */
int arroyo_amd_strkey_profile(void *h, int enable, double *last_lookup_ms);
void arroyo_amd_strkey_free_out(AmdStrBatch *out);
void arroyo_amd_strkey_destroy(void *h);
const char *arroyo_amd_strkey_last_error(void *h);

/* ---- device tuple-key dictionary: composite and NULL keys -----------------
 * Every keyed operator above takes one non-nullable i64 key column; the
 * reference keys its state on the row-encoded key tuple
 * (crates/arroyo-state/src/tables/expiring_time_key_map.rs:1008-1049), any
 * number of columns, a SQL NULL being one more key value.  This family
 * interns a tuple of n_cols (1..AMD_TKEY_MAX_COLS) 64-bit words, each with
 * an optional Arrow validity bit, on device: every tuple maps to an opaque,
 * stable, non-negative i64 id that any operator above accepts as its single
 * key column, and ids map back to columns and validity at emission.  It
 * sits in front of and behind the other operators exactly as the string-key
 * dictionary does, and no engine changes.  One handle is shared by every
 * operator that must agree on the ids (both sides of a join).  A strkey id
 * is a legal component: GROUP BY event_type, driver_id on raw strings is
 * strkey_encode, then tuplekey_encode over (string id, driver_id), the
 * operator, tuplekey_decode, then strkey_decode of the first component.
 *
 *   tuplekey_encode / _device  <-> the key row-encoding ahead of process_batch
 *   tuplekey_decode / _device  <-> rebuilding the key columns of an emission
 *   tuplekey_hash_device       <-> the key hash of the sending side of a
 *                                  keyed shuffle
 *   tuplekey_checkpoint_drain / tuplekey_restore
 *                              <-> part of the keyed operators' checkpoint:
 *                                  their drained state refers to these ids
 *
 * Columns: `cols` is n_cols pointers to columns of n_rows 8-byte elements.
 * `validity` is NULL (nothing is NULL) or n_cols pointers, each NULL (column
 * all valid) or an Arrow validity bitmap, LSB order, bit offset 0, of
 * (n_rows + 7) / 8 bytes; no byte past that is read and bits at positions
 * >= n_rows influence nothing.  A bitmap on a handle created with
 * nullable = 0 is an error.  On the device surface the pointer tables are
 * host arrays of device addresses, and a device bitmap is 8-byte aligned and
 * padded to a multiple of 8 bytes (the *_nullable_device convention).
 *
 * Identity: two tuples are equal iff their null masks are equal (one byte,
 * bit c set when component c is NULL) and their words are equal at every
 * non-NULL position.  The word under a NULL is never read, neither for
 * identity nor for the hash, and is stored and decoded as 0.  Words compare
 * as raw 64-bit patterns: for an f64 column -0.0 and 0.0 are different keys,
 * and two NaNs are one key only if their bits agree.  (NULL, 0), (0, NULL)
 * and (0, 0) are three keys.  Ids are opaque; callers may assume only
 * id >= 0 (never the engines' EMPTY_KEY), for the life of the handle and
 * across batches.
 *
 * Hash: hashes_out / d_hashes_out may be NULL; otherwise they receive the
 * 64-bit content hash per row,
 *   h = splitmix64(mask); for c in 0 .. n_cols - 1: h = splitmix64(h ^ w_c)
 * with w_c = 0 under a NULL and splitmix64 the finaliser arroyo_amd_partition
 * uses; shuffle.tuple_hash_np restates the hash in numpy.  It is
 * identical across handles, devices and hash_bits.  Ids are per handle, so a
 * keyed shuffle partitions on this hash (AMD_SHUF_KEY_HASH), never on ids;
 * tuplekey_hash_device computes it alone and touches no table state.  For a
 * Utf8 component the sender passes strkey's content-hash column as that
 * component: string ids differ per GPU, the content hash does not.
 *
 * Joins: SQL GROUP BY and PARTITION BY put all NULLs in one group, which is
 * what the identity above gives.  An equi-join never matches a NULL key: the
 * caller of a join drops rows with a NULL key component before encode (the
 * map operator's IS_NOT_NULL filter) or routes them to the unmatched output.
 * The dictionary does not decide that.
 *
 * encode: n_rows is at most 2^31 - 2 per call (more is an error);
 * n_rows == 0 succeeds and does nothing.  Rows of one batch that hold the
 * same new tuple get the same id in that call.
 *
 * decode returns n_cols host columns in `out` (free with
 * arroyo_amd_free_out).  out->validity is NULL when no decoded component is
 * NULL; otherwise it is a table with a bitmap for exactly the columns that
 * hold a NULL.  decode_device writes n_cols device columns and, on a
 * nullable = 1 handle, n_cols device bitmaps of (n_rows + 63) / 64 64-bit
 * words each, written in full, bits past n_rows clear; d_validity_out is
 * NULL on a nullable = 0 handle and required otherwise.  It is for chaining
 * behind an operator with emit_to_host = 0.  An id that is negative, out of
 * range or was never issued is an error.
 *
 * Capacity: at most 7/8 of the slots are used.  An encode that would pass
 * that fails ("capacity"); tuples interned by earlier calls stay valid, the
 * failing call's ids_out are undefined and its claimed slots are retired.
 *
 * checkpoint_drain returns every interned tuple: column 0 the ids, then the
 * n_cols components, validity by the rule of decode.  restore loads that
 * into an EMPTY handle (anything else is an error) so every tuple keeps its
 * id.  An id is a slot of the hash table, so the restoring handle needs the
 * same n_cols, log2_capacity, hash_bits and nullable; an id out of range or
 * not reachable from its tuple's home slot, or a bitmap on a nullable = 0
 * handle, is an error and leaves the handle empty.  n_cols is the length of
 * the `cols` table and cannot be checked by the callee.
 *
 * The device surface takes device pointers, runs on the handle's own stream
 * and synchronises before returning, so a chained *_process_batch_device on
 * another handle may consume d_ids_out directly.  A call allocates no device
 * memory beyond what create sized, except that the per-batch scratch grows
 * with n_rows.  One call at a time per handle.
 *
 * Out of scope: eviction (ids must stay stable for live state);
 * variable-width components other than through strkey ids; more than
 * AMD_TKEY_MAX_COLS columns; bit offsets into a bitmap; the window engine's
 * embedded composite-key dictionary is unchanged and nothing switches over
 * to this family silently; the oracle has no counterpart -- a host
 * dictionary is the checker for an interner. */
void *arroyo_amd_tuplekey_create(const AmdTupleKeyConfig *cfg);
int arroyo_amd_tuplekey_encode(void *h, const void *const *cols,
                               const uint8_t *const *validity, int64_t n_rows,
                               int64_t *ids_out, uint64_t *hashes_out);
int arroyo_amd_tuplekey_encode_device(void *h, const void *const *d_cols,
                                      const uint8_t *const *d_validity,
                                      int64_t n_rows, int64_t *d_ids_out,
                                      uint64_t *d_hashes_out);
int arroyo_amd_tuplekey_hash_device(void *h, const void *const *d_cols,
                                    const uint8_t *const *d_validity,
                                    int64_t n_rows, uint64_t *d_hashes_out);
int arroyo_amd_tuplekey_decode(void *h, const int64_t *ids, int64_t n_rows,
                               AmdOutBatch *out);
int arroyo_amd_tuplekey_decode_device(void *h, const int64_t *d_ids,
                                      int64_t n_rows, void *const *d_cols_out,
                                      uint64_t *const *d_validity_out);
int arroyo_amd_tuplekey_count(void *h, int64_t *n_tuples);
int arroyo_amd_tuplekey_checkpoint_drain(void *h, AmdOutBatch *out);
int arroyo_amd_tuplekey_restore(void *h, const int64_t *ids,
                                const void *const *cols,
                                const uint8_t *const *validity,
                                int64_t n_rows);
void arroyo_amd_tuplekey_destroy(void *h);
const char *arroyo_amd_tuplekey_last_error(void *h);

/* ---- keyed shuffle: stable device partition ------------------------------
 * The reference repartitions a batch between subtasks by sorting it by
 * destination and slicing (crates/arroyo-operator/src/context.rs:506-560);
 * the destination is the contiguous range of the key hash
 * (server_for_hash, crates/arroyo-types/src/lib.rs:640-647).  This family is
 * the device side of that: it splits a batch of up to AMD_SHUF_MAX_COLS
 * 8-byte columns, and optionally one Arrow Utf8 column, into n_parts
 * contiguous segments that can be handed to the exchange as they are.
 *
 * Owner rule: range = UINT64_MAX / n_parts + 1, owner = h / range, and
 * owner = 0 when n_parts == 1 -- the rule of arroyo_amd_partition.  h is
 * splitmix64 of the key column (AMD_SHUF_KEY_I64) or the key column itself
 * (AMD_SHUF_KEY_HASH, for the strkey content hash).
 *
 * Stable: inside a partition the rows keep their input order, and the output
 * is a pure function of the input.  An updating stream (is_retract rows)
 * relies on this: a key's append and its retraction reach the owner in the
 * order they were produced.  arroyo_amd_partition does not promise it.
 *
 * Utf8: d_offsets holds n_rows + 1 int32 entries and offsets[0] may be
 * non-zero.  A negative or decreasing offset is an error, detected on the
 * device before any byte of d_data is read; no byte outside
 * [offsets[0], offsets[n_rows]) is read.  Every partition comes out as a
 * standalone Utf8 array (see AmdShuffleOut), so a segment can be shipped and
 * passed to arroyo_amd_strkey_encode_device on the receiver without rebasing.
 * The empty string, embedded NUL bytes and non-UTF-8 bytes are legal.
 *
 * Errors (non-zero return, message in shuffle_last_error; the handle stays
 * usable and `out` is undefined): n_rows above max_rows, Utf8 bytes above
 * max_bytes, malformed offsets, a NULL column pointer, has_utf8 with a NULL
 * offsets or data pointer.  n_rows == 0 is legal: all starts are 0, every
 * partition is an empty Utf8 array and no input pointer is read.
 *
 * A call allocates no device memory and never synchronises the device: the
 * kernels run on the handle's own stream, which is synchronised once before
 * returning, so a chained *_process_batch_device or strkey_encode_device on
 * another handle may consume the outputs directly.  One call at a time per
 * handle.
 *
 * Out of scope: more than one Utf8 column; LargeUtf8 (int64 offsets);
 * validity bitmaps (a bitmap column can ride along only once widened to an
 * 8-byte column).  arroyo_amd_partition is unchanged and nothing switches
 * over to this family silently. */
void *arroyo_amd_shuffle_create(const AmdShuffleConfig *cfg);
int arroyo_amd_shuffle_partition_device(void *h, const int64_t *const *dcols,
                                        const int32_t *d_offsets,
                                        const uint8_t *d_data, int64_t n_rows,
                                        AmdShuffleOut *out);
/* Route the results of later calls into caller-owned device buffers, for an
 * exchange layer that must own the memory it sends (a torch.distributed
 * all-to-all, say): n_cols columns of max_rows entries each and, with
 * has_utf8, max_rows + n_parts offsets and max_bytes data bytes.  The
 * pointers in AmdShuffleOut are then these buffers.  d_out_cols == NULL
 * returns to the handle's own buffers, which stay allocated either way. */
int arroyo_amd_shuffle_bind_output(void *h, int64_t *const *d_out_cols,
                                   int32_t *d_out_offsets,
                                   uint8_t *d_out_data);
/* Measurement aid: enable > 0 makes every later call time its kernels with
 * HIP events, enable == 0 stops that, enable < 0 leaves the setting.
 * copy_threshold >= 0 sets the string length up to which the byte copy uses
 * one lane per string (0: the whole wave copies every string; INT32_MAX: one
 * lane per string always); < 0 leaves it.  last_kernel_ms (may be NULL)
 * receives AMD_SHUF_N_KERNELS kernel times of the last timed call. */
int arroyo_amd_shuffle_profile(void *h, int enable, int32_t copy_threshold,
                               double *last_kernel_ms);
void arroyo_amd_shuffle_destroy(void *h);
const char *arroyo_amd_shuffle_last_error(void *h);

#ifdef __cplusplus
}
#endif

#endif /* ARROYO_AMD_H */
