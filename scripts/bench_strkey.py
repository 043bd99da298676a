"""Device string-key dictionary throughput (arroyo_amd_strkey_encode_device).

Workload: 64K-row batches of 8-24-byte keys drawn uniformly from 100K
distinct strings.  Reported, all on the same GPU in one process:

  stream_gbps   arroyo_amd_stream_gbps, the streaming-read calibration
  cold          the first pass over the batches, which inserts the strings
  steady        later passes, every string known: median per-call time of
                encode_device (host clock around a call that synchronises),
                and the lookup kernel's solo time from HIP events
  host          the alternative this replaces: interning the same batches
                with a Python dict on the host, then an H2D copy of the ids

Needs a GPU; there is no CPU fallback.  Prints one JSON line.

    python scripts/bench_strkey.py [--batches 16] [--iters 30] [--warmup 3]
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
DISTINCT = 100_000


def make_batches(n_batches, seed=0):
    rng = np.random.default_rng(seed)
    pool = set()
    while len(pool) < DISTINCT:
        ln = int(rng.integers(8, 25))
        pool.add(rng.integers(33, 127, size=ln, dtype=np.uint8).tobytes())
    pool = sorted(pool)
    return [[pool[i] for i in rng.integers(0, DISTINCT, size=ROWS)]
            for _ in range(n_batches)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, default=16)
    ap.add_argument("--iters", type=int, default=30,
                    help="steady-state passes over all batches")
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_strkey needs a GPU (no CPU fallback)")
    torch.cuda.init()
    from arroyo_amd import cabi, gpu

    dev = torch.device("cuda", 0)
    batches = make_batches(args.batches)
    arrows = [cabi.strings_to_arrow(b) for b in batches]
    batch_bytes = [int(o[-1]) for o, _ in arrows]
    d_off = [torch.from_numpy(o).to(dev) for o, _ in arrows]
    d_data = [torch.from_numpy(d).to(dev) for _, d in arrows]
    d_ids = torch.empty(ROWS, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()

    n = 32 * 1024 * 1024
    a = torch.randint(0, 1 << 40, (n,), dtype=torch.int64, device=dev)
    b = torch.randint(0, 1 << 40, (n,), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    stream_gbps = gpu.lib().arroyo_amd_stream_gbps(a.data_ptr(), b.data_ptr(),
                                                   n, 20)
    del a, b

    def encode(sk, i):
        sk.encode_device(d_off[i].data_ptr(), d_data[i].data_ptr(), ROWS,
                         d_ids.data_ptr())

    # warm the code objects on a throw-away handle
    w = gpu.make_strkey(cabi.make_strkey_config(log2_capacity=18,
                                                arena_bytes=1 << 23))
    encode(w, 0)
    encode(w, 0)
    w.close()

    sk = gpu.make_strkey(cabi.make_strkey_config(log2_capacity=18,
                                                 arena_bytes=1 << 23))
    sk.profile(True)
    cold_s, cold_kernel_ms = [], []
    for i in range(args.batches):
        t0 = time.perf_counter()
        encode(sk, i)
        cold_s.append(time.perf_counter() - t0)
        cold_kernel_ms.append(sk.profile())
    n_strings = sk.count()

    for _ in range(args.warmup):
        for i in range(args.batches):
            encode(sk, i)
    call_s, kernel_ms = [], []
    for _ in range(args.iters):
        for i in range(args.batches):
            t0 = time.perf_counter()
            encode(sk, i)
            call_s.append(time.perf_counter() - t0)
            kernel_ms.append(sk.profile())
    assert sk.count() == n_strings, "steady state must insert nothing"

    # the same calls without the event pair, to show what timing costs
    sk.profile(False)
    plain_s = []
    for _ in range(max(1, args.iters // 3)):
        for i in range(args.batches):
            t0 = time.perf_counter()
            encode(sk, i)
            plain_s.append(time.perf_counter() - t0)
    sk.close()

    # host alternative: Python dict interning + H2D copy of the ids
    table = {}
    for bt in batches:                                   # cold pass
        for s in bt:
            table.setdefault(s, len(table))
    host_s = []
    for _ in range(max(1, args.iters // 10)):
        for bt in batches:
            t0 = time.perf_counter()
            ids = np.fromiter((table.setdefault(s, len(table)) for s in bt),
                              dtype=np.int64, count=ROWS)
            d_ids.copy_(torch.from_numpy(ids))
            torch.cuda.synchronize()
            host_s.append(time.perf_counter() - t0)

    mean_bytes = float(np.mean(batch_bytes))
    med = statistics.median

    def rates(seconds):
        return {"rows_per_s": ROWS / seconds,
                "key_bytes_per_s": mean_bytes / seconds}

    res = {
        "bench": "strkey_encode_device",
        "rows_per_batch": ROWS,
        "distinct_strings": DISTINCT,
        "strings_interned": n_strings,
        "mean_key_bytes_per_batch": mean_bytes,
        "stream_gbps": stream_gbps,
        "cold": {"calls": len(cold_s),
                 "first_call_ms": cold_s[0] * 1e3,
                 "median_call_ms": med(cold_s) * 1e3,
                 "median_probe_kernel_ms": med(cold_kernel_ms),
                 **rates(med(cold_s))},
        "steady": {"calls": len(call_s),
                   "median_call_ms": med(call_s) * 1e3,
                   "p10_call_ms": float(np.percentile(call_s, 10)) * 1e3,
                   "p90_call_ms": float(np.percentile(call_s, 90)) * 1e3,
                   "median_call_ms_untimed": med(plain_s) * 1e3,
                   "median_lookup_kernel_ms": med(kernel_ms),
                   "lookup_kernel": rates(med(kernel_ms) * 1e-3),
                   **rates(med(call_s))},
        "host_dict_plus_h2d": {"calls": len(host_s),
                               "median_call_ms": med(host_s) * 1e3,
                               **rates(med(host_s))},
    }
    print(json.dumps(res))


if __name__ == "__main__":
    main()
