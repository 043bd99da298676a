"""Device tuple-key dictionary throughput (arroyo_amd_tuplekey_encode_device).

Workload: 64K-row batches of n_cols i64 components, n_cols 2 and 4, with the
handle nullable off and on (on: every component NULL on a tenth of the rows,
bitmaps device-resident).  Reported per case, all on the same GPU in one
process:

  stream_gbps   arroyo_amd_stream_gbps, the streaming-read calibration, and
                the time it implies for merely reading a batch's columns
  all_new       every row of every call is a tuple the handle has never
                seen and that occurs once in the batch: 16 calls, 1M inserts
  steady        the same 16 batches again, every tuple known: median
                per-call time of encode_device (host clock around a call
                that synchronises)

Needs a GPU; there is no CPU fallback.  Prints one JSON line and sets no
pass/fail threshold.

    python scripts/bench_tuplekey.py [--batches 16] [--iters 20] [--warmup 3]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ROWS = 65536
LOG2_CAPACITY = 21      # 2M slots: 16 batches of new tuples fill half


def make_batches(n_batches, n_cols, nullable, seed):
    """Batches whose rows are distinct tuples, within and across batches:
    component 0 counts the rows, the others are random."""
    rng = np.random.default_rng(seed)
    out = []
    for b in range(n_batches):
        cols = [np.arange(b * ROWS, (b + 1) * ROWS, dtype=np.int64)]
        cols += [rng.integers(0, 1 << 40, size=ROWS).astype(np.int64)
                 for _ in range(n_cols - 1)]
        valid = None
        if nullable:
            # component 0 stays valid so the rows stay distinct tuples
            valid = [None] + [rng.random(ROWS) >= 0.1
                              for _ in range(n_cols - 1)]
        out.append((cols, valid))
    return out


def device_bitmap(mask):
    bm = np.zeros((len(mask) + 63) // 64 * 8, dtype=np.uint8)
    bm[:(len(mask) + 7) // 8] = np.packbits(mask, bitorder="little")
    return bm


def run_case(torch, cabi, gpu, dev, n_cols, nullable, args):
    batches = make_batches(args.batches, n_cols, nullable,
                           seed=10 * n_cols + nullable)
    d_cols = [[torch.from_numpy(c).to(dev) for c in cols]
              for cols, _ in batches]
    d_bm = [None if valid is None else
            [None if v is None else torch.from_numpy(device_bitmap(v)).to(dev)
             for v in valid] for _, valid in batches]
    d_ids = torch.empty(ROWS, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    cfg = lambda: cabi.make_tuplekey_config(
        n_cols, log2_capacity=LOG2_CAPACITY, nullable=nullable)

    def encode(tk, i):
        tk.encode_device(
            [t.data_ptr() for t in d_cols[i]],
            None if d_bm[i] is None else
            [None if t is None else t.data_ptr() for t in d_bm[i]],
            ROWS, d_ids.data_ptr())

    w = gpu.make_tuplekey(cfg())     # warm the code objects
    encode(w, 0)
    encode(w, 0)
    w.close()

    tk = gpu.make_tuplekey(cfg())
    new_s = []
    for i in range(args.batches):
        t0 = time.perf_counter()
        encode(tk, i)
        new_s.append(time.perf_counter() - t0)
    n_tuples = tk.count()
    assert n_tuples == args.batches * ROWS, "every row was a new tuple"

    for _ in range(args.warmup):
        for i in range(args.batches):
            encode(tk, i)
    steady_s = []
    for _ in range(args.iters):
        for i in range(args.batches):
            t0 = time.perf_counter()
            encode(tk, i)
            steady_s.append(time.perf_counter() - t0)
    assert tk.count() == n_tuples, "steady state must insert nothing"
    tk.close()

    col_bytes = ROWS * 8 * n_cols + (ROWS // 8 * (n_cols - 1) if nullable
                                     else 0)
    med = statistics.median

    def stats(seconds):
        return {"calls": len(seconds), "median_call_us": med(seconds) * 1e6,
                "p10_call_us": float(np.percentile(seconds, 10)) * 1e6,
                "p90_call_us": float(np.percentile(seconds, 90)) * 1e6,
                "rows_per_s": ROWS / med(seconds)}

    return {"n_cols": n_cols, "nullable": int(nullable),
            "input_bytes_per_batch": col_bytes,
            "tuples_interned": n_tuples,
            "all_new": {"first_call_us": new_s[0] * 1e6, **stats(new_s)},
            "steady": stats(steady_s)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=16)
    ap.add_argument("--iters", type=int, default=20,
                    help="steady-state passes over all batches")
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_tuplekey needs a GPU (no CPU fallback)")
    torch.cuda.init()
    from arroyo_amd import cabi, gpu

    dev = torch.device("cuda", 0)
    n = 32 * 1024 * 1024
    a = torch.randint(0, 1 << 40, (n,), dtype=torch.int64, device=dev)
    b = torch.randint(0, 1 << 40, (n,), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    stream_gbps = gpu.lib().arroyo_amd_stream_gbps(a.data_ptr(), b.data_ptr(),
                                                   n, 20)
    del a, b

    cases = [run_case(torch, cabi, gpu, dev, n_cols, nullable, args)
             for n_cols in (2, 4) for nullable in (False, True)]
    for c in cases:
        c["stream_read_us"] = c["input_bytes_per_batch"] / stream_gbps * 1e-3
    print(json.dumps({"bench": "tuplekey_encode_device",
                      "rows_per_batch": ROWS,
                      "log2_capacity": LOG2_CAPACITY,
                      "stream_gbps": stream_gbps, "cases": cases}))


if __name__ == "__main__":
    main()
