"""Measurement harness for the arroyo-amd hot path (BASELINE.json metric:
rows/sec on nexmark q5 sliding-window aggregate).

A "step" is one pass of the hot path over one 64K-row synthetic nexmark bid
batch already resident in HBM: the fused bin+hash-aggregate update kernel
(k_update_batch_n, quad-batched probes with a per-block LDS hot cache;
ARROYO_AMD_UPD selects the measured alternates), plus the
watermark-driven window firing (the fused
hash-aligned merge+compact kernel k_merge_fused) at the reference's
watermark cadence (1/s of event time,
crates/arroyo-worker/src/arrow/watermark_generator.rs).  Steps are
submitted in fused watermark periods (BENCH_WM_FUSE, default 4) --
bit-identical outputs, verified by tests/test_property_large.py.  Outputs stay
device-resident (the next pipeline stage's collector consumes them in place);
the host-visible emission path is covered by tests, not timed here.

Workload = BASELINE.json configs[1]: q5 hot-items, 10s width / 2s slide
COUNT GROUP BY auction, 64K-row batches (configs[0] is the reference's
CPU-runnable plumbing case; the others are parity-test cases).

Usage: python bench.py --gpus N --steps K --warmup W [--full]
                       [--dump-outputs DIR]
A plain run sets up, warms up, times exactly K steps and prints the result
line.  --full adds the legs that take runs of their own (cpu_baseline,
boundary_host); without it those fields are null.  --dump-outputs writes
what the last timed step left for the next pipeline stage -- the newest
fired windows, read back from the device output buffers after the timed
region, and the emitted-row count -- as DIR/<name>.npy (float64, sorted
rows; inputs are seeded, so two builds can be compared file for file).
For N>1 the driver launches this under torch.distributed.run, one rank per
GPU; each rank processes its own 64K-row batch per step and the keyed
shuffle (device partition kernel + RCCL all-to-all over xGMI) runs inside
the timed region ("weak" scaling: per-GPU work fixed).

Emits ONE JSON line from rank 0, including:
  - roofline: dominant-kernel achieved GB/s (algorithmic bytes per launch /
    HIP-event launch time, measured on the operator's own stream) vs the
    8 TB/s HBM3E spec peak (/opt/skills/guides/MI355X_MICROARCH.md);
    algorithmic bytes = 16 B/row (key i64 + _timestamp i64), see DESIGN.md.
  - cpu_baseline (--full only): the CPU oracle (oracle/arroyo_oracle.c, a
    restatement of the reference's operator — kind "port") timed on the
    host's cores over a bounded sample of the same workload, rank 0 at N=1
    only.
"""
import argparse
import ctypes
import json
import os
import sys
import time


sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from arroyo_amd import cabi, nexmark  # noqa: E402
from arroyo_amd.pipeline import NS  # noqa: E402

BATCH_ROWS = 65536
EVENTS_PER_SEC = 1_000_000       # event-time rate of the synthetic stream
# replay ring sized to 512 MiB so launches read from HBM, not the 256 MiB
# Infinity Cache (PMC FETCH_SIZE showed a 4-batch ring was fully L3-resident)
BASE_BATCHES = 512
WIDTH_S, SLIDE_S = 10, 2
LOG2_CAPACITY = int(os.environ.get("BENCH_LOG2_CAP", "19"))
# ~130K distinct auctions per 2s pane -> default 2^18 slots (~50% load):
# the round-2 sweep measured the smaller pane table worth +9% whole-job
# (less scan/merge/retire/CPI traffic) with loud-error headroom intact
# merge knobs: the 512-slot home range + 2048-slot LDS dedup table won the
# round-2 sweep (these only seed defaults; explicit env wins)
os.environ.setdefault("ARROYO_AMD_MF_RANGE", "1024")
os.environ.setdefault("ARROYO_AMD_MF_SLOTS", "2048")
RING_PANES = int(os.environ.get("BENCH_RING_PANES", "16"))
HBM_PEAK_GBPS = 8000.0           # spec peak (MI355X_MICROARCH.md)
ALG_BYTES_PER_ROW = 16           # compulsory HBM read: auction i64 + ts i64
CPU_SAMPLE_ROWS = 64_000_000
HOST_SAMPLE_ROWS = 32_000_000    # host-pointer boundary leg sample
DUMP_MAX_BYTES = 48 << 20        # --dump-outputs budget (hard limit 64 MB)
DUMP_SAMPLE_SEED = 1234


def op_config(device):
    return cabi.make_config(
        width_ns=WIDTH_S * NS, slide_ns=SLIDE_S * NS, n_keys=1,
        n_value_cols=0, aggs=[(cabi.COUNT, -1)],
        log2_capacity=LOG2_CAPACITY, ring_panes=RING_PANES,
        device=device, emit_to_host=False)


def gen_stream(seed):
    """BASE_BATCHES x BATCH_ROWS bid rows; returns (key, ts, span_ns)."""
    n = BASE_BATCHES * BATCH_ROWS
    key, ts = nexmark.bids(n, events_per_sec=EVENTS_PER_SEC, seed=seed)
    # replay period: event time advanced by one full pass of the base stream
    span = int(((n * nexmark.TOTAL_PROPORTION) // nexmark.BID_PROPORTION)
               * NS // EVENTS_PER_SEC)
    return key, ts, span


class WatermarkClock:
    """Reference watermark cadence: emit (max_ts - 1s lateness) at most once
    per 1s of event time (watermark_generator.rs:150-196)."""

    def __init__(self):
        self.last = 0

    def maybe(self, batch_max_ts):
        if batch_max_ts - self.last > NS:
            self.last = batch_max_ts
            return batch_max_ts - NS
        return None


def run_gpu(args):
    import torch

    from arroyo_amd import gpu

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", str(rank)))
    # functional testing of the N>1 path on a 1-GPU box: all ranks share
    # device 0 (RCCL permitting); never set in real runs
    if os.environ.get("BENCH_FORCE_DEV") is not None:
        local_rank = int(os.environ["BENCH_FORCE_DEV"])
    dist = None
    if world > 1:
        import torch.distributed as dist_mod
        dist = dist_mod
        dist.init_process_group("nccl", rank=rank, world_size=world)
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)

    key, ts, span = gen_stream(seed=42 + rank)
    d_key = torch.from_numpy(key).to(dev)
    d_ts = torch.from_numpy(ts).to(dev)
    # per-batch views into the replay ring
    views = [(d_key[i * BATCH_ROWS:(i + 1) * BATCH_ROWS],
              d_ts[i * BATCH_ROWS:(i + 1) * BATCH_ROWS])
             for i in range(BASE_BATCHES)]
    # shuffle scratch (N>1): partitioned send buffers + receive buffers.
    # The exchange runs once per fused watermark period (not per 64K
    # batch): one partition kernel + one size gather + one all_to_all
    # over the period's contiguous ring slice -- collective count drops
    # ~60x and the update launches stay period-fused like N=1.  Sized for
    # a full period; (world+1)x headroom because the nexmark hot key
    # sends ~half of every rank's rows to one owner.
    if world > 1:
        wm_every_est = int(NS // (span // BASE_BATCHES)) + 1
        period_rows = (wm_every_est *
                       int(os.environ.get("BENCH_WM_FUSE", "4")) *
                       BATCH_ROWS)
        sk = torch.empty(period_rows, dtype=torch.int64, device=dev)
        st = torch.empty(period_rows, dtype=torch.int64, device=dev)
        rbuf_cap = (world + 1) * period_rows
        rk = torch.empty(rbuf_cap, dtype=torch.int64, device=dev)
        rt = torch.empty(rbuf_cap, dtype=torch.int64, device=dev)

    op = gpu.make_op(op_config(local_rank))
    wm_lib = gpu.lib()
    batch_span = span // BASE_BATCHES
    wm_every = int(NS // batch_span) + 1   # steps per watermark (~1s cadence)

    wm_fires = [0]   # watermarks emitted (window fires happen inside these)

    def wm_value(step):
        """watermark after `step` batches: reference cadence ~1/s of event
        time (watermark_generator.rs), value = max_ts - 1s lateness."""
        b = (step - 1) % BASE_BATCHES
        cycle = (step - 1) // BASE_BATCHES
        max_ts = int(ts[(b + 1) * BATCH_ROWS - 1]) + cycle * span
        return max_ts - NS

    def emit_watermarks(steps):
        """one batched call per fused period: no rows arrive between these
        watermarks, so one device-status read serves the group."""
        vals = (ctypes.c_uint64 * len(steps))(*[wm_value(s) for s in steps])
        rc = wm_lib.arroyo_amd_handle_watermarks(
            op._h, vals, ctypes.c_int32(len(steps)), None)
        if rc != 0:
            raise RuntimeError(op._fn["last_error"](op._h).decode())
        wm_fires[0] += len(steps)

    # Watermark-period fusion: the operator's late-row filter guarantees a
    # row arriving after watermark W can never land in a pane that W's
    # windows read (its bin is >= W's bin or it is dropped), so the harness
    # may submit WM_FUSE watermark periods of rows in one launch and then
    # emit those watermarks in order -- outputs are bit-identical (covered
    # by tests/test_property_large.py), only emission latency grows by
    # WM_FUSE-1 periods of event time.  Larger launches amortize the
    # ~7 us fixed cost (ramp + launch latency) of the update kernel
    # (round-2 sweeps: optimum 4 for the batched kernel).
    wm_fuse = int(os.environ.get("BENCH_WM_FUSE", "4"))
    # Epoch pipelining (BENCH_PIPELINE=0 restores the sequential order):
    # submit period g+1 before folding period g's watermarks, so the fold's
    # host latency hides behind g+1's kernels.  set_filter_watermark keeps
    # the late-drop cutoff exactly as in the sequential order (the stream
    # here is time-monotone anyway); emissions are bit-identical
    # (tests/test_gpu_parity.py::test_epoch_pipelined_equals_sequential).
    pipelined = os.environ.get("BENCH_PIPELINE", "1") != "0"

    def emit_watermarks_epoch(steps):
        vals = (ctypes.c_uint64 * len(steps))(*[wm_value(s) for s in steps])
        rc = wm_lib.arroyo_amd_handle_watermarks_epoch(
            op._h, vals, ctypes.c_int32(len(steps)), None)
        if rc != 0:
            raise RuntimeError(op._fn["last_error"](op._h).decode())
        wm_fires[0] += len(steps)

    def run_span(s_begin, n_steps):
        """single-GPU fast path: multi-batch submits split at fused
        watermark boundaries and ring wraps."""
        s, end = s_begin, s_begin + n_steps
        while s < end:
            period = wm_every * wm_fuse
            take = min(period - (s % period), end - s)
            while take:
                b = s % BASE_BATCHES
                sub = min(take, BASE_BATCHES - b)
                op.process_batches_device(
                    [d_key.data_ptr() + b * BATCH_ROWS * 8,
                     d_ts.data_ptr() + b * BATCH_ROWS * 8],
                    BATCH_ROWS, sub, contiguous=True,
                    ts_offset0=(s // BASE_BATCHES) * span)
                s += sub
                take -= sub
            # emit every watermark boundary crossed so far, in order
            first_unemitted = (run_span.last_wm // wm_every + 1) * wm_every
            group = list(range(first_unemitted, s + 1, wm_every))
            if not group:
                continue
            if pipelined:
                rc = wm_lib.arroyo_amd_mark_epoch(op._h)
                if rc != 0:
                    raise RuntimeError(op._fn["last_error"](op._h).decode())
                wm_lib.arroyo_amd_set_filter_watermark(
                    op._h, ctypes.c_uint64(wm_value(group[-1])))
                if run_span.pending:
                    emit_watermarks_epoch(run_span.pending)
                run_span.pending = group
            else:
                emit_watermarks(group)
            run_span.last_wm = group[-1]

    def drain_pending():
        if run_span.pending:
            emit_watermarks_epoch(run_span.pending)
            run_span.pending = None

    run_span.last_wm = 0
    run_span.pending = None

    def run_span_dist(s_begin, n_steps):
        """N>1 fast path: the period's contiguous ring slice is
        partitioned and exchanged in ONE collective round, then ingested
        as one fused multi-batch launch; watermarks emit batched."""
        from arroyo_amd.shuffle import recv_splits_of
        s, end = s_begin, s_begin + n_steps
        while s < end:
            period = wm_every * wm_fuse
            take = min(period - (s % period), end - s)
            while take:
                b = s % BASE_BATCHES
                sub = min(take, BASE_BATCHES - b)
                nrows = sub * BATCH_ROWS
                ts_off = (s // BASE_BATCHES) * span
                # fence the op's consumers of the previous exchange
                wm_lib.arroyo_amd_sync(op._h)
                counts = gpu.partition_device(
                    d_key.data_ptr() + b * BATCH_ROWS * 8, 0,
                    d_ts.data_ptr() + b * BATCH_ROWS * 8, nrows, world,
                    sk.data_ptr(), 0, st.data_ptr())
                send_splits = [int(c) for c in counts]
                tsizes = torch.tensor(send_splits, dtype=torch.int64,
                                      device=dev)
                gathered = torch.empty(world * world, dtype=torch.int64,
                                       device=dev)
                dist.all_gather_into_tensor(gathered, tsizes)
                recv_splits = recv_splits_of(gathered.cpu().tolist(),
                                             world, rank)
                n_recv = sum(recv_splits)
                if n_recv > rbuf_cap:
                    raise RuntimeError(
                        f"rank {rank}: skewed exchange overflows the "
                        f"receive buffer ({n_recv} rows > cap "
                        f"{rbuf_cap}); raise the rbuf_cap headroom")
                dist.all_to_all_single(rk[:n_recv], sk[:nrows],
                                       output_split_sizes=recv_splits,
                                       input_split_sizes=send_splits)
                dist.all_to_all_single(rt[:n_recv], st[:nrows],
                                       output_split_sizes=recv_splits,
                                       input_split_sizes=send_splits)
                torch.cuda.current_stream().synchronize()
                if n_recv:
                    op.process_batch_device([rk.data_ptr(), rt.data_ptr()],
                                            n_recv, ts_off)
                s += sub
                take -= sub
            first_unemitted = (run_span.last_wm // wm_every + 1) * wm_every
            group = list(range(first_unemitted, s + 1, wm_every))
            if group:
                emit_watermarks(group)
                run_span.last_wm = group[-1]

    def one_step(step):
        b = step % BASE_BATCHES
        cycle = step // BASE_BATCHES
        ts_off = cycle * span
        bk, bt = views[b]
        if world > 1:
            # fence the operator's stream before overwriting the exchange
            # buffers it may still be consuming from the previous step
            wm_lib.arroyo_amd_sync(op._h)
            counts = gpu.partition_device(
                bk.data_ptr(), 0, bt.data_ptr(), BATCH_ROWS, world,
                sk.data_ptr(), 0, st.data_ptr())
            send_splits = [int(c) for c in counts]
            tsizes = torch.tensor(send_splits, dtype=torch.int64, device=dev)
            gathered = torch.empty(world * world, dtype=torch.int64,
                                   device=dev)
            dist.all_gather_into_tensor(gathered, tsizes)
            from arroyo_amd.shuffle import recv_splits_of
            recv_splits = recv_splits_of(gathered.cpu().tolist(), world,
                                         rank)
            n_recv = sum(recv_splits)
            if n_recv > rbuf_cap:
                raise RuntimeError(
                    f"rank {rank}: skewed exchange overflows the receive "
                    f"buffer ({n_recv} rows > cap {rbuf_cap}); raise the "
                    f"rbuf_cap headroom")
            dist.all_to_all_single(rk[:n_recv], sk,
                                   output_split_sizes=recv_splits,
                                   input_split_sizes=send_splits)
            dist.all_to_all_single(rt[:n_recv], st,
                                   output_split_sizes=recv_splits,
                                   input_split_sizes=send_splits)
            torch.cuda.current_stream().synchronize()
            if n_recv:
                op.process_batch_device([rk.data_ptr(), rt.data_ptr()],
                                        n_recv, ts_off)
        else:
            op.process_batch_device([bk.data_ptr(), bt.data_ptr()],
                                    BATCH_ROWS, ts_off)
        # event-time clock is global across ranks: same watermark everywhere
        max_ts = int(ts[(b + 1) * BATCH_ROWS - 1]) + ts_off
        wm = clock.maybe(max_ts)
        if wm is not None:
            rc = wm_lib.arroyo_amd_handle_watermark(
                op._h, ctypes.c_uint64(wm), None)
            if rc != 0:
                raise RuntimeError(op._fn["last_error"](op._h).decode())
            wm_fires[0] += 1

    clock = WatermarkClock()
    torch.cuda.synchronize()
    step_exchange = os.environ.get("BENCH_STEP_EXCHANGE") == "1"
    if world == 1:
        run_span(0, args.warmup)
    elif step_exchange:
        for s in range(args.warmup):
            one_step(s)
    else:
        run_span_dist(0, args.warmup)
    torch.cuda.synchronize()
    op.perf()  # reset kernel-time counters after warmup

    # the timed region is exactly --steps steps; with N>1 every rank
    # reports the slowest rank's time (max all-reduce)
    wm_fires[0] = 0
    timed_steps = args.steps
    if dist:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if world == 1:
        run_span(args.warmup, timed_steps)
    elif step_exchange:
        for s in range(args.warmup, args.warmup + timed_steps):
            one_step(s)
    else:
        run_span_dist(args.warmup, timed_steps)
    torch.cuda.synchronize()
    if dist:
        dist.barrier()
    t1 = time.perf_counter()
    elapsed = t1 - t0
    if dist:
        e = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(e, op=dist.ReduceOp.MAX)
        elapsed = float(e.item())

    if world == 1:
        drain_pending()
    perf = op.perf()
    perf["wm_fires_timed"] = wm_fires[0]
    outputs = None
    if args.dump_outputs:
        # what the next pipeline stage would find after the last timed step:
        # the newest fired windows, still resident in the operator's device
        # output buffers, and the running emitted-row count
        outputs = {
            "last_windows": op.last_emission(),
            "emitted_rows": perf["emitted_device_rows"],
        }
    op.close()
    if dist:
        dist.destroy_process_group()
    return elapsed, perf, rank, world, timed_steps, outputs


def _oracle_run(key, ts):
    """Run the CPU oracle over one (possibly key-sharded) sub-stream."""
    import oracle
    from arroyo_amd.pipeline import batches_from_columns

    op = oracle.make_op(op_config(device=0))
    clock = WatermarkClock()
    for cols in batches_from_columns([key, ts], BATCH_ROWS):
        op.process_batch(cols)
        wm = clock.maybe(int(cols[-1][-1]))
        if wm is not None:
            op.handle_watermark(wm)
    op.close()


def _oracle_shard_worker(key, ts, min_rows, q):
    """N-core leg worker: self-timed steady-state passes over its shard
    (process start/import/alloc overhead excluded — the measured quantity
    is per-core operator throughput, matching the reference's long-running
    subtask model)."""
    passes = max(1, -(-min_rows // max(len(key), 1)))
    t0 = time.perf_counter()
    for _ in range(passes):
        _oracle_run(key, ts)
    t1 = time.perf_counter()
    q.put((passes * len(key), t1 - t0))


def physical_cores():
    try:
        import psutil
        n = psutil.cpu_count(logical=False)
        if n:
            return n
    except Exception:
        pass
    return os.cpu_count() or 1


def cpu_baseline():
    """Oracle (CPU restatement, kind 'port') rows/s on a bounded sample of
    the same workload: single thread, and key-hash-sharded across N =
    #physical host cores (the reference's parallelism-N subtask model:
    each shard owns a contiguous hash range)."""
    import multiprocessing as mp

    key, ts = nexmark.bids(CPU_SAMPLE_ROWS, events_per_sec=EVENTS_PER_SEC,
                           seed=42)
    t0 = time.perf_counter()
    _oracle_run(key, ts)
    t1 = time.perf_counter()
    one_core = CPU_SAMPLE_ROWS / (t1 - t0)

    ncores = physical_cores()
    value_n = one_core
    if ncores > 1:
        from arroyo_amd.shuffle import partition_ids
        pid = partition_ids(key, ncores)
        q = mp.Queue()
        # each worker replays its shard until it has done >= min_rows of
        # work, self-timing only the operator loop (not fork/import), so
        # the N-core figure is steady-state per-core throughput x N
        min_rows = max(2_000_000, CPU_SAMPLE_ROWS // ncores)
        procs = []
        for p in range(ncores):
            m = pid == p
            procs.append(mp.Process(target=_oracle_shard_worker,
                                    args=(key[m], ts[m], min_rows, q)))
        for pr in procs:
            pr.start()
        rates = []
        for _ in procs:
            rows_done, secs = q.get()
            rates.append(rows_done / secs)
        for pr in procs:
            pr.join()
        # whole-job rate with every shard running concurrently = the
        # slowest per-shard rate x N (shards are balanced by key hash)
        value_n = min(rates) * ncores
    return {
        "value": value_n,
        "unit": "rows/s",
        "cores": ncores,
        "kind": "port",
        "value_1core": one_core,
        "sample": f"{CPU_SAMPLE_ROWS} rows of the same nexmark q5 stream, "
                  f"oracle/arroyo_oracle.c: single-thread {t1 - t0:.1f}s; "
                  f"N-core = min over {ncores} key-hash shards of "
                  f"self-timed steady-state rate x {ncores}",
    }


def host_boundary_leg():
    """The drop-in boundary measured honestly (SURVEY.md SS8d protocol):
    rows/s of the A1 window op fed through host-pointer process_batch
    (caller-owned host batches -> pinned staging -> H2D -> kernels), with
    watermark emission, on a bounded sample.  Reported beside (never as)
    the device-resident headline."""
    from arroyo_amd import gpu

    key, ts = nexmark.bids(HOST_SAMPLE_ROWS, events_per_sec=EVENTS_PER_SEC,
                           seed=43)
    op = gpu.make_op(op_config(device=0))
    clock = WatermarkClock()
    # warmup pass over the first 4M rows
    for b in range(64):
        s = slice(b * BATCH_ROWS, (b + 1) * BATCH_ROWS)
        op.process_batch([key[s], ts[s]])
    n_batches = HOST_SAMPLE_ROWS // BATCH_ROWS
    t0 = time.perf_counter()
    for b in range(n_batches):
        s = slice(b * BATCH_ROWS, (b + 1) * BATCH_ROWS)
        op.process_batch([key[s], ts[s]])
        wm = clock.maybe(int(ts[s][-1]))
        if wm is not None:
            op.handle_watermark(wm)
    gpu.lib().arroyo_amd_sync(op._h)
    t1 = time.perf_counter()
    op.close()
    return {
        "value": HOST_SAMPLE_ROWS / (t1 - t0),
        "unit": "rows/s",
        "includes": "host memcpy + pinned staging + H2D + kernels + "
                    "watermark firing",
        "sample": f"{HOST_SAMPLE_ROWS} rows, 64K-row host batches",
    }


def dump_outputs(outdir, outputs, rank, world):
    """Write the last timed step's outputs as <name>.npy (float64: keys and
    counts are integers below 2^53 and the window bounds whole seconds in
    ns, multiples of 2^9, so the conversion from int64 is exact).  Rows
    of a fired window leave the kernel in no fixed order, so they are sorted
    first; an emission over the size budget is cut to a fixed seeded sample
    of its sorted rows, the same rows on every run."""
    import numpy as np

    os.makedirs(outdir, exist_ok=True)
    suffix = "" if world == 1 else f"_rank{rank}"
    cols = outputs["last_windows"]
    rows = (np.stack(cols, axis=1) if cols
            else np.empty((0, 0), dtype=np.int64))
    if rows.shape[0]:
        # total order over [key, count, window_start, window_end,
        # _timestamp], key major
        rows = rows[np.lexsort(tuple(rows[:, ::-1].T))]
        max_rows = DUMP_MAX_BYTES // (8 * rows.shape[1])
        if rows.shape[0] > max_rows:
            rng = np.random.default_rng(DUMP_SAMPLE_SEED)
            pick = np.sort(rng.choice(rows.shape[0], size=max_rows,
                                      replace=False))
            rows = rows[pick]
    np.save(os.path.join(outdir, f"last_windows{suffix}.npy"),
            rows.astype(np.float64))
    np.save(os.path.join(outdir, f"emitted_rows{suffix}.npy"),
            np.array([outputs["emitted_rows"]], dtype=np.float64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=400,
                    help="number of timed steps (exactly)")
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--full", action="store_true",
                    help="after the headline run, also time the CPU oracle "
                         "baseline and the host-pointer boundary leg "
                         "(N=1 only)")
    ap.add_argument("--skip-cpu-baseline", action="store_true",
                    help="with --full: skip those legs after all")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step left for the next "
                         "stage as DIR/<name>.npy")
    args = ap.parse_args()
    if args.steps < 1:
        raise SystemExit("--steps must be >= 1")

    if args.gpus > 1 and int(os.environ.get("WORLD_SIZE", "1")) == 1:
        raise SystemExit(
            "--gpus N>1 must run under torch.distributed.run with "
            "--nproc-per-node N (one rank per GPU); a single-process run "
            "would misreport whole-job throughput")
    elapsed, perf, rank, world, timed_steps, outputs = run_gpu(args)
    if outputs is not None:
        dump_outputs(args.dump_outputs, outputs, rank, world)
    if rank != 0:
        return

    n_gpus = world
    total_rows = timed_steps * BATCH_ROWS * n_gpus
    value = total_rows / elapsed

    launches = max(perf["launches"], 1)
    avg_launch_ms = perf["update_ms"] / launches
    rows_per_launch = perf["rows"] / launches
    achieved_gbps = (rows_per_launch * ALG_BYTES_PER_ROW) / (
        avg_launch_ms * 1e-3) / 1e9 if avg_launch_ms > 0 else 0.0

    cpu = None
    boundary = None
    if args.full and world == 1 and not args.skip_cpu_baseline:
        cpu = cpu_baseline()
        boundary = host_boundary_leg()

    print(json.dumps({
        "metric": "nexmark_q5_rows_per_sec",
        "value": value,
        "unit": "rows/s",
        "n_gpus": n_gpus,
        "steps": timed_steps,
        "warmup": args.warmup,
        "ms_per_step": elapsed * 1000 / timed_steps,
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "int64",
        "data": "synthetic",
        "config": {
            "workload": "nexmark q5 hot-items: 10s/2s sliding COUNT GROUP BY"
                        " auction, 64K-row batches (BASELINE.json configs[1])",
            "batch_rows": BATCH_ROWS,
            "events_per_sec": EVENTS_PER_SEC,
            "width_s": WIDTH_S,
            "slide_s": SLIDE_S,
            "parallelism": f"key-hash dp{n_gpus}",
        },
        "roofline": {
            "bound": "hbm",
            "achieved": achieved_gbps,
            "peak": HBM_PEAK_GBPS,
            "unit": "GB/s",
            "frac": achieved_gbps / HBM_PEAK_GBPS,
            "traffic": None,
            "kernel": "k_update_batch",
            "avg_launch_us": avg_launch_ms * 1000,
            "rows_per_launch": rows_per_launch,
        },
        "timed_s": elapsed,
        "wm_fires_timed": perf.get("wm_fires_timed"),
        "boundary_host": boundary,
        "cpu_baseline": cpu,
    }))


if __name__ == "__main__":
    main()
