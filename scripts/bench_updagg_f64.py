"""Updating-aggregate ingest throughput over a Float64 column next to the
same aggregates over an i64 column (arroyo_amd_updagg_process_batch_device).

Workload: one device-resident batch of --rows rows [key, value, is_retract],
appends only, SUM + AVG + MIN + MAX over the value column, with

  uniform   keys drawn uniformly from 2**20
  skew64    every row on one of 64 keys (64 lanes of a wave meet on a
            handful of state words)

each as an i64 column (the operator as it was: SUM is an integer atomic
add, AVG folds with a compare-and-swap loop) and as an f64 column
(val_is_f64: SUM and AVG fold with the hardware f64 atomic add).  A timed
pass is `reps` process_batch_device calls of the same batch, back to back on
the operator's stream, plus one expire() with an idle bound no key reaches:
that call emits nothing and synchronises the stream, so the host clock sees
every update kernel.  `reps` is chosen per case from the warm-up so that a
pass lasts about --pass-ms (one batch of the uniform cases takes about a
millisecond, too short a window to compare two builds by).  The cost of the
synchronising call alone is reported as sync_call_us; it is paid once per
pass.

All cases run in one process, one pass of each per round in rotating order,
so a difference between two cases is neither a difference between two
processes nor one of position in the round.  With
--baseline-so PATH the i64 cases also run through another build of the
library (the parent commit's, say), interleaved in the same rounds: that is
the comparison that shows whether the i64 path moved.

Needs a GPU; there is no CPU fallback.  Prints one JSON line and sets no
pass/fail threshold.

    python scripts/bench_updagg_f64.py [--rows 4194304] [--iters 12]
        [--warmup 3] [--pass-ms 100] [--baseline-so PATH]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LOG2_KEYS = 20
NEVER = (1 << 31) - 1      # an idle bound in flushes that no key reaches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 22)
    ap.add_argument("--iters", type=int, default=12, help="timed rounds")
    ap.add_argument("--pass-ms", type=float, default=100.0,
                    help="target length of one timed pass")
    ap.add_argument("--warmup", type=int, default=3, help="untimed rounds")
    ap.add_argument("--baseline-so", default=None,
                    help="another build of libarroyo_amd.so for the i64 cases")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_updagg_f64 needs a GPU (no CPU fallback)")
    torch.cuda.init()
    from arroyo_amd import cabi, gpu

    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(7)
    n = args.rows
    keys = {"uniform": rng.integers(0, 1 << LOG2_KEYS, size=n),
            "skew64": rng.integers(0, 64, size=n)}
    vf = rng.normal(100.0, 37.0, size=n)
    vals = {"i64": np.rint(vf * 100).astype(np.int64),
            "f64": vf.view(np.int64)}
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int64)).to(dev)
    d_keys = {k: up(v) for k, v in keys.items()}
    d_vals = {k: up(v) for k, v in vals.items()}
    d_retr = torch.zeros(n, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()

    aggs = [(cabi.SUM, 0), (cabi.AVG, 0), (cabi.MIN, 0), (cabi.MAX, 0)]
    libs = {"": gpu.lib()}
    if args.baseline_so:
        libs["baseline_"] = cabi.declare(ctypes.CDLL(args.baseline_so),
                                         "arroyo_amd_")

    cases = {}
    for tag, lib in libs.items():
        for dist in keys:
            for typ in ("i64", "f64"):
                if tag and typ == "f64":
                    continue       # the other build may not know the flag
                cfg = cabi.make_updagg_config(
                    aggs, n_keys=1, n_value_cols=1,
                    log2_capacity=LOG2_KEYS + 1, log2_nodes=10,
                    log2_out_cap=10,
                    val_is_f64=(0,) if typ == "f64" else ())
                op = cabi.UpdAggOp(lib, "arroyo_amd_", cfg)
                ptrs = [d_keys[dist].data_ptr(), d_vals[typ].data_ptr(),
                        d_retr.data_ptr()]
                cases[f"{tag}{typ}_{dist}"] = [op, ptrs, [], 1, 0]

    def one_pass(case):
        op, ptrs, _, reps, _ = case
        t0 = time.perf_counter()
        for _ in range(reps):
            op.process_batch_device(ptrs, n)
        op.expire(NEVER)
        case[4] += reps
        return time.perf_counter() - t0

    for w in range(args.warmup):
        for case in cases.values():
            t = one_pass(case)
            if w == 0:
                continue           # the first pass loads the code objects
            case[3] = max(1, min(256, round(args.pass_ms * 1e-3
                                            / (t / case[3]))))
    # the two builds of a case run the same number of batches per pass
    for name, case in cases.items():
        if name.startswith("baseline_"):
            case[3] = cases[name[len("baseline_"):]][3]
    # rotate the order every round: a case's time depends a little on what
    # ran before it (a skew64 pass of the i64 column lasts half a second)
    order = list(cases.values())
    for r in range(args.iters):
        k = r % len(order)
        for case in order[k:] + order[:k]:
            case[2].append(one_pass(case))
    sync = []
    op0 = next(iter(cases.values()))[0]
    for _ in range(50):
        t0 = time.perf_counter()
        op0.expire(NEVER)
        sync.append(time.perf_counter() - t0)

    # the sums are what they should be: the figures above are of real work
    for name in ("i64_skew64", "f64_skew64"):
        passes = cases[name][4]
        out = cases[name][0].flush()
        assert len(out[0]) == 64 and not out[-1].any()
        k = int(out[0][0])
        sel = keys["skew64"] == k
        if name.startswith("i64"):
            assert int(out[1][0]) == passes * int(vals["i64"][sel].sum())
        else:
            want = passes * float(np.sum(vf[sel]))
            assert abs(float(out[1][0]) - want) <= 1e-9 * abs(want)

    result = {"bench": "updagg_f64_ingest", "rows": n, "iters": args.iters,
              "warmup": args.warmup,
              "sync_call_us": statistics.median(sync) * 1e6, "cases": {}}
    for name, (op, _, secs, reps, _) in cases.items():
        op.close()
        med = statistics.median(secs)
        result["cases"][name] = {
            "batches_per_pass": reps,
            "median_ms": med * 1e3, "min_ms": min(secs) * 1e3,
            "max_ms": max(secs) * 1e3, "rows_per_s": reps * n / med,
            "rows_per_s_best": reps * n / min(secs)}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
