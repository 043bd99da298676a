"""Loader for the MI355X product library (libarroyo_amd.so).

The HIP extension is built in-tree by __graft_entry__.build() (or lazily here
with hipcc if the source is newer).  There is NO CPU fallback: on a machine
with a GPU, operator creation either runs the HIP path or raises.
"""
import ctypes
import os
import subprocess

from arroyo_amd.cabi import (WindowOp, _batch_args, _Handle, _ptr_array,
                             declare)

_DIR = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_DIR, "libarroyo_amd.so")
_SRCS = [os.path.join(_DIR, "csrc", f)
         for f in ("arroyo_amd.hip", "join.hip", "session.hip", "expjoin.hip",
                   "updagg.hip", "windowfn.hip", "mapop.hip", "strkey.hip",
                   "shuffle.hip", "tuplekey.hip")]
# headers every source includes: editing one rebuilds the library
_HDRS = [os.path.join(_DIR, "csrc", f) for f in ("op_common.h", "op_out.h")]
_HDRS += [os.path.join(_DIR, "..", "include", f)
          for f in ("arroyo_amd_types.h", "arroyo_amd_map_check.h",
                    "arroyo_amd_map_null.h")]

_lib = None

HIPCC_CMD = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
             "-shared", "-fvisibility=hidden", "-parallel-jobs=6",
             "-o", _SO] + _SRCS


def build(force=False):
    if force or not os.path.exists(_SO) or \
            os.path.getmtime(_SO) < max(os.path.getmtime(s)
                                        for s in _SRCS + _HDRS):
        proc = subprocess.run(HIPCC_CMD, cwd=_DIR,
                              capture_output=True, text=True)
        if proc.returncode != 0:
            raise RuntimeError(
                f"hipcc failed (rc {proc.returncode}):\n{proc.stderr}")
    return _SO


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(_SO):
            build()
        _lib = declare(ctypes.CDLL(_SO), "arroyo_amd_")
    return _lib


class GpuWindowOp(WindowOp):
    """Product-path window operator (HIP, gfx950)."""

    def __init__(self, cfg):
        super().__init__(lib(), "arroyo_amd_", cfg)

    def process_batch_device(self, dev_ptrs, n_rows, ts_offset=0):
        """dev_ptrs: list of device pointers (ints) to i64 columns."""
        self._call("process_batch_device", _ptr_array(dev_ptrs),
                   len(dev_ptrs), n_rows, ts_offset)

    def process_batches_device(self, dev_ptrs, n_rows, reps, contiguous=True,
                               ts_offset0=0, ts_step=0):
        self._call("process_batches_device", _ptr_array(dev_ptrs),
                   len(dev_ptrs), n_rows, reps, 1 if contiguous else 0,
                   ts_offset0, ts_step)

    def restore(self, cols, watermark=None):
        keep, batch = _batch_args(cols)
        self._call("restore", *batch, 1 if watermark is not None else 0,
                   watermark if watermark is not None else 0)

    def last_emission(self):
        """Host copy of the window emissions still resident in the device
        output buffers (the latest fired window per fire stream), as numpy
        columns [key?, aggs..., window_start, window_end, _timestamp]."""
        return self._call_out("last_emission")

    def perf(self):
        ms = ctypes.c_double()
        rows = ctypes.c_int64()
        launches = ctypes.c_int64()
        emitted = ctypes.c_int64()
        self._call("perf", ctypes.byref(ms), ctypes.byref(rows),
                   ctypes.byref(launches), ctypes.byref(emitted))
        return {"update_ms": ms.value, "rows": rows.value,
                "launches": launches.value,
                "emitted_device_rows": emitted.value}


def make_op(cfg):
    return GpuWindowOp(cfg)


def make_join_op(cfg):
    from arroyo_amd.cabi import JoinOp
    return JoinOp(lib(), "arroyo_amd_", cfg)


def partition_device(d_keys, d_vals, d_ts, n, n_parts, d_out_keys, d_out_vals,
                     d_out_ts):
    counts = (ctypes.c_uint64 * n_parts)()
    rc = lib().arroyo_amd_partition(
        d_keys, d_vals, d_ts, n, n_parts, d_out_keys, d_out_vals, d_out_ts,
        counts)
    if rc != 0:
        raise RuntimeError("arroyo_amd_partition failed")
    return list(counts)


def make_session_op(cfg):
    from arroyo_amd.cabi import SessionOp
    return SessionOp(lib(), "arroyo_amd_", cfg)


def make_expjoin_op(cfg):
    from arroyo_amd.cabi import ExpJoinOp
    return ExpJoinOp(lib(), "arroyo_amd_", cfg)


def make_updagg_op(cfg):
    from arroyo_amd.cabi import UpdAggOp
    return UpdAggOp(lib(), "arroyo_amd_", cfg)


def make_windowfn_op(cfg):
    from arroyo_amd.cabi import WindowFnOp
    return WindowFnOp(lib(), "arroyo_amd_", cfg)


def make_map_op(cfg):
    from arroyo_amd.cabi import MapOp
    return MapOp(lib(), "arroyo_amd_", cfg)


def make_strkey(cfg):
    from arroyo_amd.cabi import StrKeyDict
    return StrKeyDict(lib(), "arroyo_amd_", cfg)


def make_tuplekey(cfg):
    from arroyo_amd.cabi import TupleKeyDict
    return TupleKeyDict(lib(), "arroyo_amd_", cfg)


class Shuffler(_Handle):
    """Stable device partition for the keyed shuffle (arroyo_amd_shuffle_*):
    up to 16 8-byte columns and optionally one Arrow Utf8 column, split
    into n_parts contiguous segments, rows of a segment in input order.

    With bind_output (the default) the results land in torch tensors this
    wrapper allocates once and binds to the handle, so partition() returns
    ordinary torch views that an exchange may send as they are.  Without it
    only partition_ptrs() is available and the results stay in the handle's
    own buffers, for chaining into another handle's *_device call."""

    FAMILY = "shuffle_"

    def __init__(self, cfg, bind_output=True):
        super().__init__(lib(), "arroyo_amd_", cfg)
        self._out = None
        if bind_output:
            import torch
            dev = torch.device("cuda", cfg.device)
            cols = [torch.empty(cfg.max_rows, dtype=torch.int64, device=dev)
                    for _ in range(cfg.n_cols)]
            off = data = None
            if cfg.has_utf8:
                off = torch.empty(cfg.max_rows + cfg.n_parts,
                                  dtype=torch.int32, device=dev)
                data = torch.empty(max(cfg.max_bytes, 1), dtype=torch.uint8,
                                   device=dev)
            self._call("bind_output",
                       _ptr_array([c.data_ptr() for c in cols]),
                       off.data_ptr() if cfg.has_utf8 else None,
                       data.data_ptr() if cfg.has_utf8 else None)
            self._out = (cols, off, data)

    def partition_ptrs(self, dev_ptrs, n_rows, d_offsets=None, d_data=None):
        """Device addresses (ints, None = NULL) in, AmdShuffleOut out; its
        device pointers are valid until the next call on this handle."""
        from arroyo_amd.cabi import AmdShuffleOut
        out = AmdShuffleOut()
        self._call("partition_device", _ptr_array(dev_ptrs), d_offsets,
                   d_data, n_rows, ctypes.byref(out))
        return out

    def partition(self, cols, utf8=None):
        """cols: n_cols equal-length contiguous 8-byte torch tensors on the
        handle's device; utf8: (int32 offsets [n + 1], uint8 data) tensors
        or None.  Returns shuffle.Partitioned whose tensors are views of
        this wrapper's output tensors, valid until the next call."""
        import torch
        from arroyo_amd.shuffle import Partitioned
        if self._out is None:
            raise RuntimeError("partition() needs bind_output=True")
        if len(cols) != self.cfg.n_cols:
            raise ValueError(f"expected {self.cfg.n_cols} columns")
        n = cols[0].numel()
        for c in cols:
            if c.numel() != n or c.element_size() != 8 or \
                    not c.is_contiguous() or not c.is_cuda:
                raise ValueError("columns must be equal-length contiguous "
                                 "8-byte device tensors")
        d_off = d_data = None
        if utf8 is not None:
            off, data = utf8
            if off.dtype != torch.int32 or off.numel() != n + 1 or \
                    data.dtype != torch.uint8 or not off.is_contiguous() or \
                    not data.is_contiguous():
                raise ValueError("utf8 = (int32 offsets [n + 1], uint8 data)")
            # a column of empty strings may come with a zero-size data
            # tensor; no byte is read then, any non-NULL address will do
            d_off, d_data = off.data_ptr(), data.data_ptr() or off.data_ptr()
        # fence torch's stream before the handle's own stream reads
        torch.cuda.current_stream(cols[0].device).synchronize()
        out = self.partition_ptrs([c.data_ptr() for c in cols], n, d_off,
                                  d_data)
        k = self.cfg.n_parts
        ocols, ooff, odata = self._out
        views = [ocols[i][:n].view(cols[i].dtype) for i in range(len(cols))]
        if utf8 is None:
            return Partitioned(views, out.row_start[:k + 1])
        return Partitioned(views, out.row_start[:k + 1], ooff[:n + k],
                           odata[:out.byte_start[k]], out.byte_start[:k + 1])

    def profile(self, enable=None, copy_threshold=None):
        """Measurement aid: switch per-kernel event timing on/off and set the
        byte-copy threshold (None leaves either); returns the kernel
        milliseconds of the last timed call by kernel name."""
        from arroyo_amd.cabi import AMD_SHUF_N_KERNELS, SHUF_KERNEL_NAMES
        ms = (ctypes.c_double * AMD_SHUF_N_KERNELS)()
        self._call("profile", -1 if enable is None else int(bool(enable)),
                   -1 if copy_threshold is None else int(copy_threshold), ms)
        return dict(zip(SHUF_KERNEL_NAMES, ms))

    def close(self):
        super().close()
        self._out = None


def make_shuffler(cfg, bind_output=True):
    return Shuffler(cfg, bind_output)
