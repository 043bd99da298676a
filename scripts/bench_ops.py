"""Supporting throughput datapoints for the non-headline operators
(profiles/): TTL join probe+insert rate and updating-aggregate update rate
on synthetic streams.  Run on a GPU box: python scripts/bench_ops.py"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np

NS = 10**9
T0 = 1_600_000_000 * NS


def bench_expjoin():
    from arroyo_amd import cabi, gpu
    rng = np.random.default_rng(1)
    n = 1 << 20
    batches = 48
    op = gpu.make_expjoin_op(cabi.make_expjoin_config(
        3600 * NS, n_left_vals=1, n_right_vals=1, log2_capacity=25,
        log2_rows_cap=26, log2_out_cap=24, emit_to_host=False))
    # ~1M keys so matches stay ~1 per probe (updating-join regime)
    def batch(i, side):
        k = rng.integers(0, 1 << 24, size=n).astype(np.int64)
        v = rng.integers(0, 100, size=n).astype(np.int64)
        ts = T0 + np.full(n, i, dtype=np.int64) * NS
        return [k, v, ts]
    data = [batch(i, i % 2) for i in range(batches)]
    t0 = time.perf_counter()
    rows = 0
    for i, cols in enumerate(data):
        out = op.process_batch(i % 2, cols)
        rows += n
    dt = time.perf_counter() - t0
    op.close()
    print(f"expjoin: {rows/dt/1e9:.3f} Grows/s ingest+probe "
          f"({dt*1e6/batches:.0f} us per 1M-row batch, ~1 match/row "
          f"by the last batches)")


def bench_updagg():
    from arroyo_amd import cabi, gpu
    rng = np.random.default_rng(2)
    n = 1 << 20
    batches = 48
    op = gpu.make_updagg_op(cabi.make_updagg_config(
        [(cabi.COUNT, -1), (cabi.SUM, 0)], n_keys=1, n_value_cols=1,
        log2_capacity=22, log2_out_cap=24))
    key = rng.integers(0, 1 << 21, size=n * 2).astype(np.int64)
    val = rng.integers(0, 1000, size=n * 2).astype(np.int64)
    retract = np.zeros(n * 2, dtype=np.int64)
    t0 = time.perf_counter()
    rows = 0
    for i in range(batches):
        lo = (i % 2) * n
        op.process_batch([key[lo:lo + n], val[lo:lo + n],
                          retract[lo:lo + n]])
        rows += n
        if i % 8 == 7:
            op.flush()
    dt = time.perf_counter() - t0
    op.close()
    print(f"updagg:  {rows/dt/1e9:.3f} Grows/s update (COUNT+SUM, 2M keys, "
          f"flush every 8 batches; {dt*1e6/batches:.0f} us per 1M-row "
          f"batch incl. H2D staging)")


def bench_expjoin_device():
    import torch
    from arroyo_amd import cabi, gpu
    rng = np.random.default_rng(3)
    n = 1 << 20
    batches = 48
    dev = torch.device("cuda", 0)
    op = gpu.make_expjoin_op(cabi.make_expjoin_config(
        3600 * NS, n_left_vals=1, n_right_vals=1, log2_capacity=25,
        log2_rows_cap=26, log2_out_cap=24, emit_to_host=False))
    tens = []
    for i in range(batches):
        k = rng.integers(0, 1 << 24, size=n).astype(np.int64)
        v = rng.integers(0, 100, size=n).astype(np.int64)
        ts = T0 + np.full(n, i, dtype=np.int64) * NS
        tens.append([torch.from_numpy(c).to(dev) for c in (k, v, ts)])
    import ctypes

    def consume():
        c = ctypes.c_int64()
        rc = op._fn["match_count"](op._h, ctypes.byref(c))
        if rc != 0:
            raise RuntimeError(op._fn["last_error"](op._h).decode())
        return int(c.value)

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    matches = 0
    for i, cols in enumerate(tens):
        op.process_batch_device(i % 2, [c.data_ptr() for c in cols], n)
        if i % 8 == 7:  # consume in place before the match buffer fills
            matches += consume()
    matches += consume()  # final count syncs the op stream
    dt = time.perf_counter() - t0
    op.close()
    print(f"expjoin (device-resident): {batches*n/dt/1e9:.3f} Grows/s "
          f"ingest+probe ({dt*1e6/batches:.0f} us per 1M-row batch, "
          f"{matches} matches consumed in place)")


def bench_updagg_device():
    import torch
    from arroyo_amd import cabi, gpu
    rng = np.random.default_rng(4)
    n = 1 << 20
    batches = 48
    dev = torch.device("cuda", 0)
    op = gpu.make_updagg_op(cabi.make_updagg_config(
        [(cabi.COUNT, -1), (cabi.SUM, 0)], n_keys=1, n_value_cols=1,
        log2_capacity=22, log2_out_cap=24))
    key = torch.from_numpy(
        rng.integers(0, 1 << 21, size=n * 2).astype(np.int64)).to(dev)
    val = torch.from_numpy(
        rng.integers(0, 1000, size=n * 2).astype(np.int64)).to(dev)
    ret = torch.zeros(n * 2, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(batches):
        lo = (i % 2) * n * 8
        op.process_batch_device([key.data_ptr() + lo, val.data_ptr() + lo,
                                 ret.data_ptr() + lo], n)
        if i % 8 == 7:
            op.flush()
    op.flush()  # drains the op stream (no-op emission if nothing changed)
    dt = time.perf_counter() - t0
    op.close()
    print(f"updagg (device-resident):  {batches*n/dt/1e9:.3f} Grows/s "
          f"update (COUNT+SUM, 2M keys, flush every 8 batches, "
          f"{dt*1e6/batches:.0f} us per 1M-row batch)")


def updagg_device_rate(null_semantics, null_frac=0.0, min_seconds=1.0,
                       windows=3):
    """The updagg_device shape (COUNT+SUM, 2M keys, 1M-row device-resident
    batches, a flush every 8), warmed up with 48 batches and then timed over
    `windows` windows of at least `min_seconds` each.  null_semantics=False
    drives process_batch_device, True process_batch_nullable_device with
    `null_frac` of the value column NULL.  Returns us per 1M-row batch, one
    figure per window (host clock around a window that ends in a flush, i.e.
    a stream synchronise)."""
    import torch
    from arroyo_amd import cabi, gpu
    rng = np.random.default_rng(4)
    n = 1 << 20
    dev = torch.device("cuda", 0)
    op = gpu.make_updagg_op(cabi.make_updagg_config(
        [(cabi.COUNT, -1), (cabi.SUM, 0)], n_keys=1, n_value_cols=1,
        log2_capacity=22, log2_out_cap=24, null_semantics=null_semantics))
    key = torch.from_numpy(
        rng.integers(0, 1 << 21, size=n * 2).astype(np.int64)).to(dev)
    val = torch.from_numpy(
        rng.integers(0, 1000, size=n * 2).astype(np.int64)).to(dev)
    ret = torch.zeros(n * 2, dtype=torch.int64, device=dev)
    # n is a multiple of 64, so the second half's bitmap is 8-byte aligned
    bm = torch.from_numpy(
        cabi.pack_validity(rng.random(n * 2) >= null_frac)).to(dev)
    torch.cuda.synchronize()

    def run(batches):
        for i in range(batches):
            lo = (i % 2) * n
            ptrs = [key.data_ptr() + lo * 8, val.data_ptr() + lo * 8,
                    ret.data_ptr() + lo * 8]
            if null_semantics:
                op.process_batch_nullable_device(
                    ptrs, [None, bm.data_ptr() + lo // 8, None], n)
            else:
                op.process_batch_device(ptrs, n)
            if i % 8 == 7:
                op.flush()

    run(48)
    out = []
    for _ in range(windows):
        done = 0
        t0 = time.perf_counter()
        while True:
            run(48)
            done += 48
            dt = time.perf_counter() - t0
            if dt >= min_seconds:
                break
        out.append(dt * 1e6 / done)
    op.close()
    return out


def bench_updagg_nullable_device(which=("plain", "0", "10")):
    """Nullable device-resident ingest against the non-nullable path at the
    same commit, same shape and same method.  which: "plain" = the
    null_semantics=0 path, "0" / "10" = nullable with that % of NULLs."""
    import json
    legs = {"plain": ("updagg_device (null_semantics=0)", False, 0.0),
            "0": ("updagg_nullable_device 0% NULL", True, 0.0),
            "10": ("updagg_nullable_device 10% NULL", True, 0.10)}
    for name, ns, frac in (legs[w] for w in which):
        us = updagg_device_rate(ns, frac)
        print(f"{name}: {np.median(us):.0f} us per 1M-row batch "
              f"({(1 << 20) / np.median(us) / 1e3:.3f} Grows/s; windows "
              f"{', '.join(f'{u:.0f}' for u in us)} us)")
        print(json.dumps({"leg": "updagg_nullable_device", "name": name,
                          "null_semantics": int(ns), "null_frac": frac,
                          "us_per_1M_windows": us}))


def bench_ordered(which=("A", "B"), reps=10, warmup=2):
    """Updating aggregate with per-key value multisets: 2^16 keys x ~100
    distinct values per key.  Config A = COUNT + COUNT DISTINCT (no
    order-statistic pre-pass is launched), B = A + MEDIAN + MIN_RETRACT +
    MAX_RETRACT.  Times are host-clock around calls that end in a stream
    synchronise (the operator owns its stream).  Every timed flush follows a
    one-row-per-key batch, so it re-evaluates all 2^16 keys."""
    import json
    from arroyo_amd import cabi, gpu
    n_keys = 1 << 16
    per_key = 256
    n = 1 << 20
    rng = np.random.default_rng(6)
    total = n_keys * per_key
    key = rng.permutation(np.repeat(np.arange(n_keys, dtype=np.int64),
                                    per_key))
    val = rng.integers(0, 100, size=total).astype(np.int64)
    zeros = np.zeros(n, dtype=np.int64)
    tkey = np.arange(n_keys, dtype=np.int64)
    aggs = {"A": [(cabi.COUNT, -1), (cabi.COUNT_DISTINCT, 0)]}
    aggs["B"] = aggs["A"] + [(cabi.MEDIAN, 0), (cabi.MIN_RETRACT, 0),
                             (cabi.MAX_RETRACT, 0)]
    for name in which:
        op = gpu.make_updagg_op(cabi.make_updagg_config(
            aggs[name], n_keys=1, n_value_cols=1, log2_capacity=17,
            log2_nodes=23 if name == "A" else 25, log2_out_cap=18))
        upd = []
        for lo in range(0, total, n):
            t0 = time.perf_counter()
            op.process_batch([key[lo:lo + n], val[lo:lo + n], zeros])
            upd.append((time.perf_counter() - t0) * 1e3)
        op.flush()
        fl = []
        for i in range(warmup + reps):
            tv = rng.integers(0, 100, size=n_keys).astype(np.int64)
            op.process_batch([tkey, tv, zeros[:n_keys]])
            t0 = time.perf_counter()
            out = op.flush()
            fl.append((time.perf_counter() - t0) * 1e3)
            assert len(out[0]) == 2 * n_keys   # every key re-emitted
        op.close()
        upd, fl = upd[warmup:], fl[warmup:]
        res = {"leg": "ordered", "config": name, "keys": n_keys,
               "rows": total,
               "update_ms_per_1M_median": float(np.median(upd)),
               "update_ms_per_1M_min": float(np.min(upd)),
               "update_ms_per_1M_max": float(np.max(upd)),
               "flush_ms_median": float(np.median(fl)),
               "flush_ms_min": float(np.min(fl)),
               "flush_ms_max": float(np.max(fl))}
        print(f"ordered {name}: update {res['update_ms_per_1M_median']:.2f} "
              f"ms per 1M-row batch (incl. H2D staging), flush of 2^16 "
              f"changed keys {res['flush_ms_median']:.2f} ms "
              f"(min {res['flush_ms_min']:.2f}, max {res['flush_ms_max']:.2f}"
              f", incl. D2H of the emitted rows)")
        print(json.dumps(res))


def bench_window_update(which=("tile", "batch"), streams=("uniform", "nexmark"),
                        n=54 * 65536, launches=24, windows=5):
    """The window operator's COUNT update kernel alone, one 3.5M-row
    device-resident launch at a time (the bench's fused launch size), per
    ARROYO_AMD_UPD flavour.  "uniform" draws keys uniformly over 2^20 -- no
    time locality, so a per-block table finds nothing to combine; "nexmark"
    is the bench stream.  The same rows are replayed, so after the warm-up
    every key is resident in its pane table.  Prints us per launch for each
    of `windows` timed windows (host clock around `launches` launches that
    end in a stream synchronise)."""
    import torch
    from arroyo_amd import cabi, gpu, nexmark
    dev = torch.device("cuda", 0)
    lib = gpu.lib()
    nkey, ts = nexmark.bids(n, seed=42)
    ukey = np.random.default_rng(5).integers(0, 1 << 20, size=n).astype(np.int64)
    d_ts = torch.from_numpy(ts).to(dev)
    for stream in streams:
        d_key = torch.from_numpy(ukey if stream == "uniform" else nkey).to(dev)
        for upd in which:
            os.environ["ARROYO_AMD_UPD"] = upd
            op = gpu.make_op(cabi.make_config(
                width_ns=10 * NS, slide_ns=2 * NS, n_keys=1, n_value_cols=0,
                aggs=[(cabi.COUNT, -1)], log2_capacity=22, ring_panes=16,
                emit_to_host=False))
            ptrs = [d_key.data_ptr(), d_ts.data_ptr()]
            us = []
            for w in range(windows + 1):          # window 0 warms up
                lib.arroyo_amd_sync(op._h)
                t0 = time.perf_counter()
                for _ in range(launches):
                    op.process_batch_device(ptrs, n)
                lib.arroyo_amd_sync(op._h)
                if w:
                    us.append((time.perf_counter() - t0) * 1e6 / launches)
            op.close()
            print(f"window_update {stream} {upd}: us per {n}-row launch "
                  f"{' '.join(f'{u:.1f}' for u in us)} "
                  f"(median {float(np.median(us)):.1f})")
    os.environ.pop("ARROYO_AMD_UPD", None)


LEGS = {"expjoin": bench_expjoin, "updagg": bench_updagg,
        "window_update": bench_window_update,
        "expjoin_device": bench_expjoin_device,
        "updagg_device": bench_updagg_device,
        "updagg_nullable_device": bench_updagg_nullable_device,
        "ordered": bench_ordered}


if __name__ == "__main__":
    # torch's bundled HIP runtime must initialize before the op library's
    # (system-ROCm) runtime touches the device, or torch.cuda breaks
    import torch
    torch.zeros(1, device="cuda")
    # python scripts/bench_ops.py [leg ...]; "ordered:A" runs one config
    for arg in sys.argv[1:] or list(LEGS):
        leg, _, cfgs = arg.partition(":")
        if cfgs:
            LEGS[leg](which=tuple(cfgs.split(",")))
        else:
            LEGS[leg]()
