"""Per-batch GPU time of a q1-shaped filtered map (price * 0.908 as f64 ->
i64, keep auction % 3 != 1) at 1 << 20 rows on the device surface, between
HIP events around calls that end in their own stream synchronise: the plain
path, the nullable path with every input valid, and the nullable path with
about 10% NULLs in the price column.  The cases alternate inside one process;
the figures behind profiles/nullable_map_note.md.

    python scripts/bench_null_map.py [--parent-lib OTHER/libarroyo_amd.so]

--parent-lib adds the plain path of another build of the library (the parent
commit's, built with the same hipcc flags) to the alternation."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from arroyo_amd import cabi, gpu  # noqa: E402
from arroyo_amd.cabi import (MOP_CONST, MOP_F2I, MOP_FMUL, MOP_I2F, MOP_MOD,  # noqa
                             MOP_NE)

N = 1 << 20
REPS, WARM = 300, 20

lib = gpu.lib()
rt = ctypes.CDLL(gpu._SO)
vp = ctypes.c_void_p
rt.hipMalloc.argtypes = [ctypes.POINTER(vp), ctypes.c_size_t]
rt.hipMemcpy.argtypes = [vp, vp, ctypes.c_size_t, ctypes.c_int]
rt.hipEventCreate.argtypes = [ctypes.POINTER(vp)]
rt.hipEventRecord.argtypes = [vp, vp]
rt.hipEventSynchronize.argtypes = [vp]
rt.hipEventElapsedTime.argtypes = [ctypes.POINTER(ctypes.c_float), vp, vp]


def upload(a):
    a = np.ascontiguousarray(a)
    p = vp()
    assert rt.hipMalloc(ctypes.byref(p), max(a.nbytes, 8)) == 0
    assert rt.hipMemcpy(p, a.ctypes.data, a.nbytes, 1) == 0
    return p.value


prog = [(MOP_I2F, 1, 0, 3), (MOP_CONST, 0, 0, 4, 0.908), (MOP_FMUL, 3, 4, 5),
        (MOP_F2I, 5, 0, 6), (MOP_CONST, 0, 0, 7, 3), (MOP_MOD, 0, 7, 8),
        (MOP_CONST, 0, 0, 9, 1), (MOP_NE, 8, 9, 10)]


def cfg(ns):
    return cabi.make_map_config(3, prog, [0, 6, 2], filter_reg=10,
                                null_semantics=ns)


rng = np.random.default_rng(0)
auction = rng.integers(0, 10**6, size=N).astype(np.int64)
price = rng.integers(1, 10**7, size=N).astype(np.int64)
ts = np.arange(N, dtype=np.int64)
d = [upload(auction), upload(price), upload(ts)]


def bitmap(mask):
    bm = np.packbits(mask, bitorder="little")
    pad = np.zeros((len(bm) + 7) // 8 * 8, dtype=np.uint8)
    pad[:len(bm)] = bm
    return upload(pad)


ones = bitmap(np.ones(N, dtype=bool))
ten = bitmap(rng.random(N) >= 0.1)

ap = argparse.ArgumentParser()
ap.add_argument("--parent-lib", default=None)
args = ap.parse_args()
ops = {}
if args.parent_lib:
    parent_lib = cabi.declare(ctypes.CDLL(args.parent_lib), "arroyo_amd_")
    ops["parent_plain"] = cabi.MapOp(parent_lib, "arroyo_amd_", cfg(0))
ops["plain"] = gpu.make_map_op(cfg(0))
ops["nullable_all_valid"] = gpu.make_map_op(cfg(1))
ops["nullable_10pct_null"] = gpu.make_map_op(cfg(1))


def call(name):
    op = ops[name]
    if name.endswith("plain"):
        return op.process_batch_device(d, N)[1]
    if name == "nullable_all_valid":
        return op.process_batch_nullable_device(d, [None, ones, None], N)[3]
    return op.process_batch_nullable_device(d, [None, ten, None], N)[3]


e0, e1 = vp(), vp()
rt.hipEventCreate(ctypes.byref(e0))
rt.hipEventCreate(ctypes.byref(e1))
times = {k: [] for k in ops}
kept = {}
for rep in range(WARM + REPS):
    for name in ops:
        rt.hipEventRecord(e0, None)
        kept[name] = call(name)       # ends in the call's own synchronise
        rt.hipEventRecord(e1, None)
        rt.hipEventSynchronize(e1)
        ms = ctypes.c_float()
        rt.hipEventElapsedTime(ctypes.byref(ms), e0, e1)
        if rep >= WARM:
            times[name].append(ms.value)
res = {"n_rows": N, "reps": REPS, "kept": kept}
for k, v in times.items():
    v.sort()
    res[k] = {"median_ms": statistics.median(v), "p10_ms": v[len(v) // 10],
              "p90_ms": v[len(v) * 9 // 10], "min_ms": v[0]}
print(json.dumps(res, indent=1))
