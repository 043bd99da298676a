"""Stable device shuffle (arroyo_amd_shuffle_partition_device) per-call cost.

All on one GPU in one process:

  stream_gbps   arroyo_amd_stream_gbps, the streaming-read calibration
  fixed         the q5 exchange shape: 3 i64 columns (auction, price, ts) of
                nexmark bids, 8 partitions, 64Ki and 1Mi rows per call.  The
                new call and arroyo_amd_partition (the unordered 3-column
                path, the baseline) run alternately on the same device
                buffers; host clock around calls that end synchronised, plus
                the new family's per-kernel times from HIP events, taken in a
                separate loop.
  utf8          1Mi rows, a 64-bit hash key (KEY_HASH), a timestamp column
                and one Utf8 column of mean length ~12 and ~200 bytes; the
                byte copy with its default threshold (a lane per string up
                to 32 bytes, the wave above), with a lane per string always,
                and with the wave always.

Bytes: `payload` counts every carried column once in and once out (and the
string bytes and offsets likewise); `traffic` adds what the kernels move on
top (key re-read, owner plane, length/source/position planes).

Needs a GPU; there is no CPU fallback.  Prints one JSON line.

    python scripts/bench_shuffle.py [--iters 100] [--warmup 10]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PARTS = 8
med = statistics.median


def summary(seconds):
    return {"calls": len(seconds),
            "median_call_ms": med(seconds) * 1e3,
            "p10_call_ms": float(np.percentile(seconds, 10)) * 1e3,
            "p90_call_ms": float(np.percentile(seconds, 90)) * 1e3}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--utf8-rows", type=int, default=1 << 20)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_shuffle needs a GPU (no CPU fallback)")
    torch.cuda.init()
    from arroyo_amd import cabi, gpu, nexmark
    from arroyo_amd.shuffle import KEY_HASH, KEY_I64, partition_host

    dev = torch.device("cuda", 0)
    to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    n = 32 * 1024 * 1024
    a = torch.randint(0, 1 << 40, (n,), dtype=torch.int64, device=dev)
    b = torch.randint(0, 1 << 40, (n,), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    stream_gbps = gpu.lib().arroyo_amd_stream_gbps(a.data_ptr(), b.data_ptr(),
                                                   n, 20)
    del a, b
    res = {"bench": "shuffle_partition_device", "n_parts": PARTS,
           "stream_gbps": stream_gbps, "fixed": [], "utf8": []}

    # ---- fixed-width leg ---------------------------------------------------
    for rows in (1 << 16, 1 << 20):
        cols = nexmark.bids(rows, with_price=True)
        d_in = [to_dev(c) for c in cols]
        d_old = [torch.empty(rows, dtype=torch.int64, device=dev)
                 for _ in range(3)]
        sh = gpu.make_shuffler(cabi.make_shuffle_config(
            PARTS, 3, key_col=0, key_mode=KEY_I64, max_rows=rows))
        ptrs = [t.data_ptr() for t in d_in]
        torch.cuda.synchronize()

        def old():
            return gpu.partition_device(*ptrs, rows, PARTS,
                                        *[t.data_ptr() for t in d_old])

        def new():
            return sh.partition_ptrs(ptrs, rows)

        # same answer first: counts, and the stable order against the host
        want = partition_host(cols, 0, KEY_I64, PARTS)
        counts = old()
        part = sh.partition(d_in)
        assert part.row_start == want.row_start
        assert counts == list(np.diff(want.row_start))
        for g, w in zip(part.cols, want.cols):
            assert np.array_equal(g.cpu().numpy(), w)

        for _ in range(args.warmup):
            old()
            new()
        t_old, t_new = [], []
        for _ in range(args.iters):         # alternating, same buffers
            t0 = time.perf_counter()
            old()
            t1 = time.perf_counter()
            new()
            t2 = time.perf_counter()
            t_old.append(t1 - t0)
            t_new.append(t2 - t1)
        sh.profile(True)
        kern = {k: [] for k in cabi.SHUF_KERNEL_NAMES[:3]}
        for _ in range(max(10, args.iters // 4)):
            new()
            ms = sh.profile()
            for k in kern:
                kern[k].append(ms[k])
        sh.close()
        kern_ms = {k: med(v) for k, v in kern.items()}
        payload = 2 * 3 * 8 * rows
        traffic = payload + (8 + 1 + 1) * rows      # key re-read, owner plane
        old_traffic = payload + (8 + 4 + 4) * rows  # key re-read, u32 ids
        s_new, s_old = med(t_new), med(t_old)
        k_s = sum(kern_ms.values()) * 1e-3
        res["fixed"].append({
            "rows": rows,
            "new": {**summary(t_new), "rows_per_s": rows / s_new,
                    "payload_gbps": payload / s_new / 1e9,
                    "traffic_gbps": traffic / s_new / 1e9,
                    "kernel_ms": kern_ms,
                    "kernels_total_ms": k_s * 1e3,
                    "traffic_gbps_kernels": traffic / k_s / 1e9,
                    "share_of_stream_kernels": traffic / k_s / 1e9 /
                    stream_gbps},
            "arroyo_amd_partition": {**summary(t_old),
                                     "rows_per_s": rows / s_old,
                                     "payload_gbps": payload / s_old / 1e9,
                                     "traffic_gbps": old_traffic / s_old /
                                     1e9},
            "new_over_old_call_time": s_new / s_old})

    # ---- Utf8 leg ------------------------------------------------------------
    rows = args.utf8_rows
    rng = np.random.default_rng(1)
    hashes = rng.integers(0, 1 << 63, size=rows, dtype=np.uint64) * 2
    ts = np.arange(rows, dtype=np.int64)
    d_cols = [to_dev(hashes), to_dev(ts)]
    for lo, hi in ((8, 17), (100, 301)):
        lens = rng.integers(lo, hi, size=rows)
        off = np.zeros(rows + 1, dtype=np.int64)
        np.cumsum(lens, out=off[1:])
        total = int(off[-1])
        off = off.astype(np.int32)
        data = rng.integers(33, 127, size=total, dtype=np.uint8)
        d_off, d_data = to_dev(off), to_dev(data)
        sh = gpu.make_shuffler(cabi.make_shuffle_config(
            PARTS, 2, key_col=0, key_mode=KEY_HASH, has_utf8=True,
            max_rows=rows, max_bytes=total))
        ptrs = [t.data_ptr() for t in d_cols]
        torch.cuda.synchronize()

        def call():
            return sh.partition_ptrs(ptrs, rows, d_off.data_ptr(),
                                     d_data.data_ptr())

        part = sh.partition(d_cols, (d_off, d_data))
        if total < (1 << 26):       # full check where the host copy is cheap
            want = partition_host([hashes, ts], 0, KEY_HASH, PARTS,
                                  (off, data))
            assert part.row_start == want.row_start
            assert part.byte_start == want.byte_start
            assert np.array_equal(part.utf8_offsets.cpu().numpy(),
                                  want.utf8_offsets)
            assert np.array_equal(part.utf8_data.cpu().numpy(),
                                  want.utf8_data)
        else:                       # starts only
            want = partition_host([hashes, lens.astype(np.int64)], 0,
                                  KEY_HASH, PARTS)
            assert part.row_start == want.row_start
            bs = np.concatenate([[0], np.cumsum(want.cols[1])])
            assert part.byte_start == [int(bs[r]) for r in want.row_start]

        leg = {"rows": rows, "mean_len": total / rows, "string_bytes": total,
               "schemes": {}}
        payload = 2 * (2 * 8 * rows + 4 * rows + total)
        # + key re-read, owner plane (w+r), three 4-byte planes (w+r), the
        # source offsets read twice more (count, scatter)
        traffic = payload + (8 + 2 + 3 * 8 + 8) * rows
        schemes = (("lane_up_to_32_then_wave", 32), ("lane_always", 2**31 - 1),
                   ("wave_always", 0))
        for name, thr in schemes:
            sh.profile(False, copy_threshold=thr)
            for _ in range(max(3, args.warmup // 2)):
                call()
            t = []
            for _ in range(max(10, args.iters // 4)):
                t0 = time.perf_counter()
                call()
                t.append(time.perf_counter() - t0)
            sh.profile(True)
            kern = {k: [] for k in cabi.SHUF_KERNEL_NAMES}
            for _ in range(10):
                call()
                ms = sh.profile()
                for k in kern:
                    kern[k].append(ms[k])
            kern_ms = {k: med(v) for k, v in kern.items()}
            s = med(t)
            k_s = sum(kern_ms.values()) * 1e-3
            leg["schemes"][name] = {
                **summary(t), "rows_per_s": rows / s,
                "string_bytes_per_s": total / s,
                "payload_gbps": payload / s / 1e9,
                "kernel_ms": kern_ms, "kernels_total_ms": k_s * 1e3,
                "traffic_gbps_kernels": traffic / k_s / 1e9,
                "share_of_stream_kernels": traffic / k_s / 1e9 / stream_gbps,
                "copy_kernel_string_gbps":
                    2 * total / (kern_ms["utf8_copy"] * 1e-3) / 1e9}
        sh.close()
        del d_off, d_data
        res["utf8"].append(leg)

    print(json.dumps(res))


if __name__ == "__main__":
    main()
