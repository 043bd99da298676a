"""ctypes bindings for the arroyo-amd C ABI (include/arroyo_amd.h).

Generic over the implementing library: the product HIP library
(libarroyo_amd.so, prefix ``arroyo_amd_``) and the CPU oracle
(oracle/liboracle.so, prefix ``oracle_``) export the same operator families;
tests drive both through the wrapper classes below and compare.

Layout of this file: the struct mirrors of include/arroyo_amd_types.h with
their ``make_*_config`` helpers, then PROTOTYPES (every function of
include/arroyo_amd.h, once), then ``_Handle`` and one thin wrapper class per
family.  tests/test_cabi.py checks the mirrors and the table against the
two headers.
"""
import ctypes

import numpy as np

NS = 10**9
U64MAX = 2**64 - 1

COUNT, SUM, MIN, MAX, AVG = 0, 1, 2, 3, 4


class AmdWindowConfig(ctypes.Structure):
    _fields_ = [
        ("width_nanos", ctypes.c_uint64),
        ("slide_nanos", ctypes.c_uint64),
        ("is_tumbling", ctypes.c_int32),
        ("n_keys", ctypes.c_int32),
        ("n_aggs", ctypes.c_int32),
        ("agg_ops", ctypes.c_int32 * 8),
        ("agg_col", ctypes.c_int32 * 8),
        ("n_value_cols", ctypes.c_int32),
        ("log2_capacity", ctypes.c_uint32),
        ("ring_panes", ctypes.c_uint32),
        ("device", ctypes.c_int32),
        ("emit_to_host", ctypes.c_int32),
        ("val_is_f64", ctypes.c_int32 * 8),
    ]


class AmdOutBatch(ctypes.Structure):
    _fields_ = [
        ("n_rows", ctypes.c_int64),
        ("n_cols", ctypes.c_int32),
        ("cols", ctypes.POINTER(ctypes.c_void_p)),
        ("is_f64", ctypes.POINTER(ctypes.c_int32)),
        ("on_device", ctypes.c_int32),
        ("validity", ctypes.POINTER(ctypes.POINTER(ctypes.c_uint8))),
    ]


def make_config(width_ns, slide_ns, aggs, n_keys=1, n_value_cols=0,
                is_tumbling=False, log2_capacity=20, ring_panes=64,
                device=0, emit_to_host=True, val_is_f64=()):
    """aggs: list of (op, value_col_index); value_col_index -1 for COUNT(*).
    val_is_f64: indices of value columns holding f64 bit patterns."""
    cfg = AmdWindowConfig()
    cfg.width_nanos = width_ns
    cfg.slide_nanos = width_ns if is_tumbling else slide_ns
    cfg.is_tumbling = 1 if is_tumbling else 0
    cfg.n_keys = n_keys
    cfg.n_aggs = len(aggs)
    for i, (op, col) in enumerate(aggs):
        cfg.agg_ops[i] = op
        cfg.agg_col[i] = col
    cfg.n_value_cols = n_value_cols
    for v in val_is_f64:
        cfg.val_is_f64[v] = 1
    cfg.log2_capacity = log2_capacity
    cfg.ring_panes = ring_panes
    cfg.device = device
    cfg.emit_to_host = 1 if emit_to_host else 0
    return cfg


class AmdJoinConfig(ctypes.Structure):
    _fields_ = [
        ("n_keys", ctypes.c_int32),
        ("n_left_vals", ctypes.c_int32),
        ("n_right_vals", ctypes.c_int32),
        ("log2_rows_cap", ctypes.c_uint32),
        ("instants", ctypes.c_uint32),
        ("log2_out_cap", ctypes.c_uint32),
        ("device", ctypes.c_int32),
        ("emit_to_host", ctypes.c_int32),
        ("join_type", ctypes.c_int32),
    ]


JOIN_INNER, JOIN_LEFT, JOIN_RIGHT, JOIN_FULL = 0, 1, 2, 3


def make_join_config(n_keys=1, n_left_vals=0, n_right_vals=0,
                     log2_rows_cap=15, instants=128, log2_out_cap=20,
                     device=0, emit_to_host=True, join_type=JOIN_INNER):
    cfg = AmdJoinConfig()
    cfg.n_keys = n_keys
    cfg.n_left_vals = n_left_vals
    cfg.n_right_vals = n_right_vals
    cfg.log2_rows_cap = log2_rows_cap
    cfg.instants = instants
    cfg.log2_out_cap = log2_out_cap
    cfg.device = device
    cfg.emit_to_host = 1 if emit_to_host else 0
    cfg.join_type = join_type
    return cfg


class AmdSessionConfig(ctypes.Structure):
    _fields_ = [
        ("n_keys", ctypes.c_int32),
        ("n_value_cols", ctypes.c_int32),
        ("n_aggs", ctypes.c_int32),
        ("agg_ops", ctypes.c_int32 * 8),
        ("agg_col", ctypes.c_int32 * 8),
        ("gap_nanos", ctypes.c_uint64),
        ("log2_capacity", ctypes.c_uint32),
        ("max_sessions", ctypes.c_uint32),
        ("log2_batch_capacity", ctypes.c_uint32),
        ("log2_out_cap", ctypes.c_uint32),
        ("log2_distinct", ctypes.c_uint32),
        ("log2_cd_regions", ctypes.c_uint32),
        ("device", ctypes.c_int32),
        ("emit_to_host", ctypes.c_int32),
    ]


def make_session_config(gap_ns, aggs, n_keys=1, n_value_cols=0,
                        log2_capacity=16, max_sessions=8,
                        log2_batch_capacity=14, log2_out_cap=20,
                        log2_distinct=10, log2_cd_regions=18,
                        device=0, emit_to_host=True):
    cfg = AmdSessionConfig()
    cfg.n_keys = n_keys
    cfg.n_value_cols = n_value_cols
    cfg.n_aggs = len(aggs)
    for i, (op, col) in enumerate(aggs):
        cfg.agg_ops[i] = op
        cfg.agg_col[i] = col
    cfg.gap_nanos = gap_ns
    cfg.log2_capacity = log2_capacity
    cfg.max_sessions = max_sessions
    cfg.log2_batch_capacity = log2_batch_capacity
    cfg.log2_out_cap = log2_out_cap
    cfg.log2_distinct = log2_distinct
    cfg.log2_cd_regions = log2_cd_regions
    cfg.device = device
    cfg.emit_to_host = 1 if emit_to_host else 0
    return cfg


class AmdExpJoinConfig(ctypes.Structure):
    _fields_ = [
        ("n_keys", ctypes.c_int32),
        ("n_left_vals", ctypes.c_int32),
        ("n_right_vals", ctypes.c_int32),
        ("ttl_nanos", ctypes.c_uint64),
        ("log2_capacity", ctypes.c_uint32),
        ("log2_rows_cap", ctypes.c_uint32),
        ("log2_out_cap", ctypes.c_uint32),
        ("device", ctypes.c_int32),
        ("emit_to_host", ctypes.c_int32),
        ("join_type", ctypes.c_int32),
        ("updating", ctypes.c_int32),
    ]


def make_expjoin_config(ttl_ns, n_left_vals=0, n_right_vals=0,
                        log2_capacity=16, log2_rows_cap=20, log2_out_cap=20,
                        device=0, emit_to_host=True, join_type=0,
                        updating=False):
    cfg = AmdExpJoinConfig()
    cfg.n_keys = 1
    cfg.n_left_vals = n_left_vals
    cfg.n_right_vals = n_right_vals
    cfg.ttl_nanos = ttl_ns
    cfg.log2_capacity = log2_capacity
    cfg.log2_rows_cap = log2_rows_cap
    cfg.log2_out_cap = log2_out_cap
    cfg.device = device
    cfg.emit_to_host = 1 if emit_to_host else 0
    cfg.join_type = join_type
    cfg.updating = 1 if updating else 0
    return cfg


COUNT_DISTINCT = 5
STDDEV = 6
STDDEV_POP = 7
VAR = 8
VAR_POP = 9
BIT_XOR = 10
COVAR_POP = 11
COVAR_SAMP = 12
CORR = 13
REGR_SLOPE = 14
REGR_INTERCEPT = 15
REGR_R2 = 16
REGR_AVGX = 17
REGR_AVGY = 18
REGR_COUNT = 19
REGR_SXX = 20
REGR_SYY = 21
REGR_SXY = 22
BIT_AND = 23
BIT_OR = 24
# order statistics under retraction (updating aggregate only)
MEDIAN = 25
MIN_RETRACT = 26
MAX_RETRACT = 27


class AmdUpdatingConfig(ctypes.Structure):
    _fields_ = [
        ("n_keys", ctypes.c_int32),
        ("n_value_cols", ctypes.c_int32),
        ("n_aggs", ctypes.c_int32),
        ("agg_col2", ctypes.c_int32 * 8),
        ("agg_ops", ctypes.c_int32 * 8),
        ("agg_col", ctypes.c_int32 * 8),
        ("log2_capacity", ctypes.c_uint32),
        ("log2_nodes", ctypes.c_uint32),
        ("log2_out_cap", ctypes.c_uint32),
        ("device", ctypes.c_int32),
        ("emit_to_host", ctypes.c_int32),
        ("val_is_f64", ctypes.c_int32 * 8),
        ("null_semantics", ctypes.c_int32),
    ]


def make_updagg_config(aggs, n_keys=1, n_value_cols=0, log2_capacity=16,
                       log2_nodes=20, log2_out_cap=20, device=0,
                       emit_to_host=True, null_semantics=False,
                       val_is_f64=()):
    """null_semantics=True: SQL NULL semantics (nullable value columns in,
    validity bitmaps out; see AmdUpdatingConfig in arroyo_amd_types.h).
    val_is_f64: indices of value columns holding f64 bit patterns."""
    cfg = AmdUpdatingConfig()
    cfg.n_keys = n_keys
    cfg.n_value_cols = n_value_cols
    cfg.n_aggs = len(aggs)
    for i, spec in enumerate(aggs):
        op, col = spec[0], spec[1]
        cfg.agg_ops[i] = op
        cfg.agg_col[i] = col
        cfg.agg_col2[i] = spec[2] if len(spec) > 2 else -1
    cfg.log2_capacity = log2_capacity
    cfg.log2_nodes = log2_nodes
    cfg.log2_out_cap = log2_out_cap
    cfg.device = device
    cfg.emit_to_host = 1 if emit_to_host else 0
    cfg.null_semantics = 1 if null_semantics else 0
    for v in val_is_f64:
        cfg.val_is_f64[v] = 1
    return cfg


class AmdWindowFnConfig(ctypes.Structure):
    _fields_ = [
        ("n_cols", ctypes.c_int32),
        ("part_col", ctypes.c_int32),
        ("n_order", ctypes.c_int32),
        ("order_col", ctypes.c_int32 * 2),
        ("order_desc", ctypes.c_int32 * 2),
        ("limit", ctypes.c_int64),
        ("log2_rows_cap", ctypes.c_uint32),
        ("instants", ctypes.c_uint32),
        ("log2_out_cap", ctypes.c_uint32),
        ("device", ctypes.c_int32),
        ("emit_to_host", ctypes.c_int32),
        ("fn", ctypes.c_int32),
        ("arg_col", ctypes.c_int32),
        ("frame", ctypes.c_int32),
        ("offset", ctypes.c_int64),
        ("has_default", ctypes.c_int32),
        ("default_value", ctypes.c_int64),
    ]


# AMD_WFN_* of include/arroyo_amd_types.h
(WFN_ROW_NUMBER, WFN_RANK, WFN_DENSE_RANK, WFN_LAG, WFN_LEAD,
 WFN_FIRST_VALUE, WFN_LAST_VALUE, WFN_SUM, WFN_COUNT, WFN_MIN,
 WFN_MAX) = range(11)
WFN_FRAME_RANGE, WFN_FRAME_ROWS, WFN_FRAME_PARTITION = range(3)
WFN_SCAN_TILE = 2048


def make_windowfn_config(n_cols, part_col, order, limit=0, log2_rows_cap=15,
                         instants=128, log2_out_cap=20, device=0,
                         emit_to_host=True, fn=WFN_ROW_NUMBER, arg_col=-1,
                         frame=WFN_FRAME_RANGE, offset=1, default=None):
    """order: list of (col, desc) pairs, max 2.  fn: a WFN_* function over
    the i64 column arg_col (-1 where it takes none); frame: a WFN_FRAME_*
    for the aggregates, FIRST_VALUE and LAST_VALUE; offset and default: the
    LAG/LEAD distance and the value where it leaves the partition (None =
    SQL NULL).  See AmdWindowFnConfig in arroyo_amd_types.h."""
    cfg = AmdWindowFnConfig()
    cfg.fn = fn
    cfg.arg_col = arg_col
    cfg.frame = frame
    cfg.offset = offset
    cfg.has_default = 0 if default is None else 1
    cfg.default_value = 0 if default is None else default
    cfg.n_cols = n_cols
    cfg.part_col = part_col
    cfg.n_order = len(order)
    for i, (col, desc) in enumerate(order):
        cfg.order_col[i] = col
        cfg.order_desc[i] = 1 if desc else 0
    cfg.limit = limit
    cfg.log2_rows_cap = log2_rows_cap
    cfg.instants = instants
    cfg.log2_out_cap = log2_out_cap
    cfg.device = device
    cfg.emit_to_host = 1 if emit_to_host else 0
    return cfg


MOP_CONST, MOP_ADD, MOP_SUB, MOP_MUL, MOP_DIV, MOP_MOD = range(6)
MOP_EQ, MOP_NE, MOP_LT, MOP_LE, MOP_GT, MOP_GE = range(6, 12)
MOP_AND, MOP_OR, MOP_NOT, MOP_I2F, MOP_F2I = range(12, 17)
MOP_FADD, MOP_FSUB, MOP_FMUL, MOP_FDIV = range(17, 21)
# null_semantics=1 programs only; SELECT's else-register goes in imm
MOP_IS_NULL, MOP_IS_NOT_NULL, MOP_COALESCE, MOP_NULLIF, MOP_SELECT = \
    range(21, 26)


class AmdMapInstr(ctypes.Structure):
    _fields_ = [("op", ctypes.c_int32), ("a", ctypes.c_int32),
                ("b", ctypes.c_int32), ("dst", ctypes.c_int32),
                ("imm", ctypes.c_int64)]


class AmdMapConfig(ctypes.Structure):
    _fields_ = [
        ("n_in_cols", ctypes.c_int32),
        ("n_prog", ctypes.c_int32),
        ("prog", AmdMapInstr * 64),
        ("n_out", ctypes.c_int32),
        ("out_reg", ctypes.c_int32 * 16),
        ("out_is_f64", ctypes.c_int32 * 16),
        ("filter_reg", ctypes.c_int32),
        ("device", ctypes.c_int32),
        ("emit_to_host", ctypes.c_int32),
        ("null_semantics", ctypes.c_int32),
    ]


def make_map_config(n_in_cols, prog, out_reg, out_is_f64=None,
                    filter_reg=-1, device=0, null_semantics=0):
    """prog: list of (op, a, b, dst[, imm]) tuples.  imm may be a float for
    MOP_CONST feeding f64 ops (stored as the f64 bit pattern); for
    MOP_SELECT it is the else-branch register.  null_semantics=1: SQL NULL
    semantics (validity per register, opcodes 21..25; see AmdMapConfig in
    arroyo_amd_types.h)."""
    import struct
    cfg = AmdMapConfig()
    cfg.n_in_cols = n_in_cols
    cfg.n_prog = len(prog)
    for i, ins in enumerate(prog):
        op, a, b, dst = ins[:4]
        imm = ins[4] if len(ins) > 4 else 0
        if isinstance(imm, float):
            imm = struct.unpack("<q", struct.pack("<d", imm))[0]
        cfg.prog[i].op = op
        cfg.prog[i].a = a
        cfg.prog[i].b = b
        cfg.prog[i].dst = dst
        cfg.prog[i].imm = imm
    cfg.n_out = len(out_reg)
    for i, r in enumerate(out_reg):
        cfg.out_reg[i] = r
        cfg.out_is_f64[i] = 1 if (out_is_f64 and out_is_f64[i]) else 0
    cfg.filter_reg = filter_reg
    cfg.device = device
    cfg.emit_to_host = 1
    cfg.null_semantics = int(null_semantics)
    return cfg


# ---- device string-key dictionary (arroyo_amd_strkey_*) -------------------

class AmdStrKeyConfig(ctypes.Structure):
    _fields_ = [
        ("device", ctypes.c_int32),
        ("log2_capacity", ctypes.c_int32),
        ("arena_bytes", ctypes.c_int64),
        ("hash_bits", ctypes.c_int32),
    ]


class AmdStrBatch(ctypes.Structure):
    _fields_ = [
        ("n_rows", ctypes.c_int64),
        ("ids", ctypes.POINTER(ctypes.c_int64)),
        ("offsets", ctypes.POINTER(ctypes.c_int32)),
        ("data", ctypes.POINTER(ctypes.c_uint8)),
    ]


def make_strkey_config(log2_capacity=16, arena_bytes=1 << 24, hash_bits=0,
                       device=0):
    cfg = AmdStrKeyConfig()
    cfg.device = device
    cfg.log2_capacity = log2_capacity
    cfg.arena_bytes = arena_bytes
    cfg.hash_bits = hash_bits
    return cfg


# ---- device tuple-key dictionary (arroyo_amd_tuplekey_*) -------------------

AMD_TKEY_MAX_COLS = 8
AMD_TKEY_BLOCK_THREADS = 256
AMD_TKEY_MAX_BLOCKS = 2048
# rows one pass of the largest grid covers; one more runs the stride loop twice
TKEY_GRID_ROWS = AMD_TKEY_BLOCK_THREADS * AMD_TKEY_MAX_BLOCKS
TKEY_MAX_ROWS = 2**31 - 2


class AmdTupleKeyConfig(ctypes.Structure):
    _fields_ = [
        ("device", ctypes.c_int32),
        ("n_cols", ctypes.c_int32),
        ("log2_capacity", ctypes.c_int32),
        ("hash_bits", ctypes.c_int32),
        ("nullable", ctypes.c_int32),
    ]


def make_tuplekey_config(n_cols, log2_capacity=16, hash_bits=0,
                         nullable=False, device=0):
    cfg = AmdTupleKeyConfig()
    cfg.device = device
    cfg.n_cols = n_cols
    cfg.log2_capacity = log2_capacity
    cfg.hash_bits = hash_bits
    cfg.nullable = 1 if nullable else 0
    return cfg


# ---- keyed shuffle: stable device partition (arroyo_amd_shuffle_*) --------

AMD_SHUF_KEY_I64 = 0    # owner from splitmix64 of the key column
AMD_SHUF_KEY_HASH = 1   # the key column already is a 64-bit hash
AMD_SHUF_MAX_COLS = 16
AMD_SHUF_MAX_PARTS = 64
AMD_SHUF_MAX_ROWS = 1 << 30
AMD_SHUF_N_KERNELS = 5
AMD_SHUF_TILE_ROWS = 1024
SHUF_KERNEL_NAMES = ("count", "scan", "scatter", "utf8_offsets", "utf8_copy")


class AmdShuffleConfig(ctypes.Structure):
    _fields_ = [
        ("device", ctypes.c_int32),
        ("n_parts", ctypes.c_int32),
        ("n_cols", ctypes.c_int32),
        ("key_col", ctypes.c_int32),
        ("key_mode", ctypes.c_int32),
        ("has_utf8", ctypes.c_int32),
        ("max_rows", ctypes.c_int64),
        ("max_bytes", ctypes.c_int64),
    ]


class AmdShuffleOut(ctypes.Structure):
    _fields_ = [
        ("n_rows", ctypes.c_int64),
        ("cols", ctypes.c_void_p * AMD_SHUF_MAX_COLS),
        ("utf8_offsets", ctypes.c_void_p),
        ("utf8_data", ctypes.c_void_p),
        ("row_start", ctypes.c_int64 * (AMD_SHUF_MAX_PARTS + 1)),
        ("byte_start", ctypes.c_int64 * (AMD_SHUF_MAX_PARTS + 1)),
    ]


def make_shuffle_config(n_parts, n_cols, key_col=0, key_mode=AMD_SHUF_KEY_I64,
                        has_utf8=False, max_rows=1 << 20, max_bytes=0,
                        device=0):
    cfg = AmdShuffleConfig()
    cfg.device = device
    cfg.n_parts = n_parts
    cfg.n_cols = n_cols
    cfg.key_col = key_col
    cfg.key_mode = key_mode
    cfg.has_utf8 = 1 if has_utf8 else 0
    cfg.max_rows = max_rows
    cfg.max_bytes = max_bytes
    return cfg


# ---- prototypes: every function of include/arroyo_amd.h, once -------------
#
# PROTOTYPES maps the name after the library prefix to (restype, argtypes).
# A new entry point gets one line here; tests/test_cabi.py holds the table
# against the header (same names, same parameter counts).

_P = ctypes.POINTER
_int, _i32, _i64, _u64 = (ctypes.c_int, ctypes.c_int32, ctypes.c_int64,
                          ctypes.c_uint64)
_dbl, _vp = ctypes.c_double, ctypes.c_void_p   # _vp: handle or raw address
_cols, _out, _strs = _P(_vp), _P(AmdOutBatch), _P(AmdStrBatch)

# the recurring shapes (int return unless said otherwise)
_H = (_vp,)                                    # handle
_BATCH = (_vp, _cols, _i32, _i64)              # handle, columns, count, rows
_SIDE_BATCH = (_vp, _i32, _cols, _i32, _i64)   # handle, side, columns, ...
_NULLABLE = (_vp, _cols, _cols, _i32, _i64)    # columns + validity bitmaps
_WM_OUT = (_vp, _u64, _out)                    # handle, watermark, out
_WMS_OUT = (_vp, _P(_u64), _i32, _out)         # handle, watermarks, n, out
_OUT = (_vp, _out)                             # handle, out
_SEL_OUT = (_vp, _i32, _out)                   # handle, side / which, out
_RESTORE_WM = (_int, _u64)                     # has_watermark, watermark

_FAMILIES = {   # symbol infix -> config struct of its create
    "": AmdWindowConfig, "join_": AmdJoinConfig,
    "session_": AmdSessionConfig, "expjoin_": AmdExpJoinConfig,
    "updagg_": AmdUpdatingConfig, "windowfn_": AmdWindowFnConfig,
    "map_": AmdMapConfig, "strkey_": AmdStrKeyConfig,
    "shuffle_": AmdShuffleConfig, "tuplekey_": AmdTupleKeyConfig,
}

_INT_PROTOTYPES = {
    # sliding / tumbling window aggregate
    "process_batch": _BATCH,
    "process_batch_device": _BATCH + (_u64,),
    "process_batches_device": _BATCH + (_i32, _i32, _u64, _u64),
    "sync": _H,
    "handle_watermark": _WM_OUT,
    "handle_watermarks": _WMS_OUT,
    "set_filter_watermark": (_vp, _u64),
    "mark_epoch": _H,
    "handle_watermarks_epoch": _WMS_OUT,
    "checkpoint_drain": _OUT,
    "restore": _BATCH + _RESTORE_WM,
    "perf": (_vp, _P(_dbl), _P(_i64), _P(_i64), _P(_i64)),
    "last_emission": _OUT,
    "partition": (_vp,) * 3 + (_i64, ctypes.c_uint32) + (_vp,) * 3 +
                 (_P(_u64),),
    # instant join
    "join_process_batch": _SIDE_BATCH,
    "join_process_batch_device": _SIDE_BATCH,
    "join_handle_watermark": _WM_OUT,
    "join_checkpoint_drain": _SEL_OUT,
    # session window aggregate
    "session_process_batch": _BATCH,
    "session_process_batch_device": _BATCH + (_u64,),
    "session_handle_watermark": _WM_OUT,
    "session_checkpoint_drain": _OUT,
    "session_drain_values": _OUT,
    "session_restore_values": _BATCH,
    "session_restore": _BATCH,
    # join with expiration
    "expjoin_process_batch": _SIDE_BATCH + (_out,),
    "expjoin_process_batch_device": _SIDE_BATCH,
    "expjoin_collect": _OUT,
    "expjoin_handle_watermark": (_vp, _u64),
    "expjoin_match_count": (_vp, _P(_i64)),
    "expjoin_expire": _H,
    "expjoin_checkpoint_drain": _SEL_OUT,
    "expjoin_restore": _SIDE_BATCH + _RESTORE_WM,
    # updating aggregate
    "updagg_process_batch": _BATCH,
    "updagg_process_batch_device": _BATCH,
    "updagg_process_batch_nullable": _NULLABLE,
    "updagg_process_batch_nullable_device": _NULLABLE,
    "updagg_flush": _OUT,
    "updagg_expire": (_vp, _i64, _out),
    "updagg_checkpoint_drain": _SEL_OUT,
    "updagg_restore": _SIDE_BATCH,
    # ROW_NUMBER window function
    "windowfn_process_batch": _BATCH,
    "windowfn_process_batch_device": _BATCH,
    "windowfn_restore": _BATCH,
    "windowfn_handle_watermark": _WM_OUT,
    "windowfn_checkpoint_drain": _OUT,
    # map / filter / projection
    "map_process_batch": _BATCH + (_out,),
    "map_process_batch_device": _BATCH + (_cols, _P(_i64)),
    "map_process_batch_nullable": _NULLABLE + (_out,),
    "map_process_batch_nullable_device":
        _NULLABLE + (_cols, _cols, _P(_i64), _P(_i64)),
    # string-key dictionary (buffers go in as raw addresses)
    "strkey_encode": (_vp, _vp, _vp, _i64, _vp, _vp),
    "strkey_encode_device": (_vp, _vp, _vp, _i64, _vp, _vp),
    "strkey_decode": (_vp, _vp, _i64, _strs),
    "strkey_count": (_vp, _P(_i64), _P(_i64)),
    "strkey_checkpoint_drain": (_vp, _strs),
    "strkey_restore": (_vp, _vp, _vp, _vp, _i64),
    "strkey_profile": (_vp, _int, _P(_dbl)),
    # tuple-key dictionary (column / bitmap tables, buffers as raw addresses)
    "tuplekey_encode": (_vp, _cols, _cols, _i64, _vp, _vp),
    "tuplekey_encode_device": (_vp, _cols, _cols, _i64, _vp, _vp),
    "tuplekey_hash_device": (_vp, _cols, _cols, _i64, _vp),
    "tuplekey_decode": (_vp, _vp, _i64, _out),
    "tuplekey_decode_device": (_vp, _vp, _i64, _cols, _cols),
    "tuplekey_count": (_vp, _P(_i64)),
    "tuplekey_checkpoint_drain": _OUT,
    "tuplekey_restore": (_vp, _vp, _cols, _cols, _i64),
    # keyed shuffle
    "shuffle_partition_device": (_vp, _cols, _vp, _vp, _i64,
                                 _P(AmdShuffleOut)),
    "shuffle_bind_output": (_vp, _cols, _vp, _vp),
    "shuffle_profile": (_vp, _int, _i32, _P(_dbl)),
}

PROTOTYPES = {name: (_int, args) for name, args in _INT_PROTOTYPES.items()}
PROTOTYPES["stream_gbps"] = (_dbl, (_vp, _vp, _i64, _int))
PROTOTYPES["free_out"] = (None, (_out,))
PROTOTYPES["strkey_free_out"] = (None, (_strs,))
for _infix, _cfg in _FAMILIES.items():
    PROTOTYPES[_infix + "create"] = (_vp, (_P(_cfg),))
    PROTOTYPES[_infix + "destroy"] = (None, _H)
    PROTOTYPES[_infix + "last_error"] = (ctypes.c_char_p, _H)
del _infix, _cfg


def declare(lib, prefix):
    """Give every PROTOTYPES function that `lib` exports its restype and
    argtypes.  ctypes keeps one function object per name and CDLL, so from
    here on ``lib.<prefix><name>`` is safe to call from anywhere.  Entries
    the library lacks are skipped one by one (the oracle has no device,
    nullable, epoch, strkey or shuffle entry points)."""
    for name, (restype, argtypes) in PROTOTYPES.items():
        f = getattr(lib, prefix + name, None)
        if f is not None:
            f.restype, f.argtypes = restype, argtypes
    lib.__dict__["_declared_prefix"] = prefix
    return lib


class _FamilyFns(dict):
    """{short name: function} of one family; a name the library does not
    export raises the AttributeError ctypes itself would."""

    def __init__(self, symbol_prefix):
        super().__init__()
        self._symbol_prefix = symbol_prefix

    def __missing__(self, name):
        raise AttributeError(
            f"undefined symbol: {self._symbol_prefix}{name}")


def _family_of(name):
    """The infix a table name starts with ("" for the window family)."""
    return next((i for i in _FAMILIES if i and name.startswith(i)), "")


def _family_fns(lib, prefix, infix):
    """The functions of the family `infix` that `lib` exports, by the name
    after the infix, plus the shared free_out."""
    if lib.__dict__.get("_declared_prefix") != prefix:
        declare(lib, prefix)
    fn = _FamilyFns(prefix + infix)
    for name in PROTOTYPES:
        if _family_of(name) == infix and hasattr(lib, prefix + name):
            fn[name[len(infix):]] = getattr(lib, prefix + name)
    fn.setdefault("free_out", getattr(lib, prefix + "free_out"))
    return fn


def bind(lib, prefix):
    return _family_fns(lib, prefix, "")


def bind_join(lib, prefix):
    return _family_fns(lib, prefix, "join_")


def bind_shuffle(lib, prefix="arroyo_amd_"):
    """The shuffle family; returns {name: function}."""
    return _family_fns(lib, prefix, "shuffle_")


# ---- batches in and out -----------------------------------------------------

def out_validity(out):
    """Decode the Arrow validity bitmaps of an AmdOutBatch into per-column
    numpy bool masks (None = column all-valid)."""
    n = out.n_rows
    masks = []
    if not out.validity:
        return [None] * out.n_cols
    for i in range(out.n_cols):
        bm = out.validity[i]
        if not bm:
            masks.append(None)
            continue
        nbytes = (n + 7) // 8
        raw = np.frombuffer(
            bytes(ctypes.cast(bm, ctypes.POINTER(
                ctypes.c_uint8 * max(nbytes, 1))).contents),
            dtype=np.uint8)
        masks.append(np.unpackbits(raw, bitorder="little")[:n].astype(bool))
    return masks


def pack_validity(mask):
    """Pack a bool mask into an Arrow validity bitmap (LSB bit order, bit
    offset 0, (n + 7) // 8 bytes, padding bits clear): the inverse of
    :func:`out_validity`."""
    mask = np.ascontiguousarray(mask, dtype=bool)
    return np.packbits(mask, bitorder="little")


def _out_to_numpy(out):
    """Copy an AmdOutBatch (host memory) into numpy arrays the caller owns;
    the batch may be freed once this returns."""
    n = out.n_rows
    cols = []
    for i in range(out.n_cols):
        dt = np.float64 if out.is_f64[i] else np.int64
        if n == 0:
            cols.append(np.empty(0, dtype=dt))
            continue
        view = (ctypes.c_int64 * n).from_address(out.cols[i])
        cols.append(np.frombuffer(view, dtype=dt).copy())
    return cols


def _ptr_array(ptrs):
    """void*[] over raw addresses (ints; None = NULL)."""
    return (ctypes.c_void_p * len(ptrs))(*ptrs)


def _cols_to_ptrs(cols):
    """Contiguous int64 copies + a void* array over them."""
    keep = [np.ascontiguousarray(c, dtype=np.int64) for c in cols]
    return keep, _ptr_array([c.ctypes.data for c in keep])


def _batch_args(cols):
    """The (columns, count, rows) arguments of a host batch, and the arrays
    they point into (hold these until the call has returned)."""
    keep, arr = _cols_to_ptrs(cols)
    return keep, (arr, len(keep), len(keep[0]) if keep else 0)


def _validity_args(valid, n_cols, n_rows):
    """The validity argument of a nullable host batch: `valid` is None
    (everything valid) or a list parallel to the columns of None (column
    all valid) / bool arrays (True = non-null).  Returns the packed bitmaps
    (hold these until the call has returned) and the pointer array."""
    if valid is None:
        return [], None
    if len(valid) != n_cols:
        raise ValueError(f"valid has {len(valid)} entries for {n_cols} cols")
    keep, ptrs = [], []
    for m in valid:
        if m is None:
            ptrs.append(None)
            continue
        if len(m) != n_rows:
            raise ValueError("validity mask length != n_rows")
        bm = pack_validity(m)
        if len(bm) == 0:
            bm = np.zeros(1, dtype=np.uint8)
        keep.append(bm)
        ptrs.append(bm.ctypes.data)
    return keep, _ptr_array(ptrs)


class _Handle:
    """One operator handle of the family FAMILY (the symbol infix) behind
    the C ABI: create on construction, destroy on close.  `_h` is the raw
    handle (None once closed), `_fn` the family's functions by short name,
    `cfg` the config struct the handle was created from."""

    FAMILY = ""
    _h = None

    def __init__(self, lib, prefix, cfg):
        self._fn = _family_fns(lib, prefix, self.FAMILY)
        self.cfg = cfg
        self._h = self._fn["create"](ctypes.byref(cfg))
        if not self._h:
            raise RuntimeError(
                f"{prefix}{self.FAMILY}create failed: "
                f"{self._fn['last_error'](None).decode()}")

    def _check(self, rc):
        if rc != 0:
            raise RuntimeError(self._fn["last_error"](self._h).decode())

    def _call(self, name, *args):
        self._check(self._fn[name](self._h, *args))

    def _call_out(self, name, *args, with_validity=False):
        """Call a function whose last parameter is an AmdOutBatch*; return
        its columns as numpy arrays (with with_validity: (cols, masks), a
        column without a bitmap all True) and free the batch."""
        out = AmdOutBatch()
        self._call(name, *args, ctypes.byref(out))
        cols = _out_to_numpy(out)
        masks = out_validity(out) if with_validity else None
        self._fn["free_out"](ctypes.byref(out))
        if not with_validity:
            return cols
        n = len(cols[0]) if cols else 0
        return cols, [np.ones(n, dtype=bool) if m is None else m
                      for m in masks]

    def _send(self, name, cols, *lead):
        """Call a (handle, *lead, columns, count, rows) function on a host
        batch; returns the arrays that were sent."""
        keep, batch = _batch_args(cols)
        self._call(name, *lead, *batch)
        return keep

    def close(self):
        if self._h:
            self._fn["destroy"](self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class WindowOp(_Handle):
    """One window-aggregate operator instance behind the C ABI.

    Mirrors the ArrowOperator calling convention
    (crates/arroyo-operator/src/operator.rs:1144-1257): process_batch
    ingests an owned batch; handle_watermark may emit result batches;
    single-threaded per handle."""

    def process_batch(self, cols):
        """cols: list of np.int64 arrays [keys..., values..., _timestamp].
        Returns the arrays that were sent."""
        return self._send("process_batch", cols)

    def handle_watermark(self, wm):
        return self._call_out("handle_watermark", wm)

    def handle_watermarks(self, wms):
        """Batched watermarks with no rows between them: one device-status
        round trip serves the whole group.  Semantically identical to
        handle_watermark in order; returns all emissions concatenated.
        Falls back to a Python loop where the library lacks the entry
        point (the oracle)."""
        if "handle_watermarks" not in self._fn:
            outs = [self.handle_watermark(w) for w in wms]
            outs = [o for o in outs if o and len(o[0])]
            if not outs:
                return []
            return [np.concatenate([o[c] for o in outs])
                    for c in range(len(outs[0]))]
        return self._call_out("handle_watermarks",
                              (ctypes.c_uint64 * len(wms))(*wms), len(wms))

    def set_filter_watermark(self, wm):
        self._call("set_filter_watermark", wm)

    def mark_epoch(self):
        self._call("mark_epoch")

    def handle_watermarks_epoch(self, wms):
        return self._call_out("handle_watermarks_epoch",
                              (ctypes.c_uint64 * len(wms))(*wms), len(wms))

    def checkpoint_drain(self):
        return self._call_out("checkpoint_drain")


class JoinOp(_Handle):
    """One instant-join operator instance behind the C ABI (left = side 0,
    right = side 1), mirroring InstantJoin's ArrowOperator surface
    (crates/arroyo-worker/src/arrow/instant_join.rs)."""

    FAMILY = "join_"
    LEFT, RIGHT = 0, 1

    def process_batch(self, side, cols):
        return self._send("process_batch", cols, side)

    def handle_watermark(self, wm):
        return self._call_out("handle_watermark", wm)

    def checkpoint_drain(self, side):
        return self._call_out("checkpoint_drain", side)

    def restore(self, side, cols):
        """on_start re-processes drained batches (instant_join.rs:205-230)."""
        if cols and len(cols[0]):
            self.process_batch(side, cols)


class SessionOp(_Handle):
    """One session-window aggregate operator behind the C ABI, mirroring
    SessionAggregatingWindowFunc's ArrowOperator surface
    (crates/arroyo-worker/src/arrow/session_aggregating_window.rs)."""

    FAMILY = "session_"

    def process_batch(self, cols):
        self._send("process_batch", cols)

    def handle_watermark(self, wm):
        return self._call_out("handle_watermark", wm)

    def checkpoint_drain(self):
        return self._call_out("checkpoint_drain")

    def restore(self, cols):
        self._send("restore", cols)

    def drain_values(self):
        """GPU-only extension (the oracle drains raw rows instead)."""
        return self._call_out("drain_values")

    def restore_values(self, cols):
        self._send("restore_values", cols)


class ExpJoinOp(_Handle):
    """One TTL'd (non-windowed) join operator behind the C ABI, mirroring
    JoinWithExpiration's ArrowOperator surface
    (crates/arroyo-worker/src/arrow/join_with_expiration.rs)."""

    FAMILY = "expjoin_"
    LEFT, RIGHT = 0, 1

    def process_batch(self, side, cols):
        keep, batch = _batch_args(cols)
        return self._call_out("process_batch", side, *batch)

    def handle_watermark(self, wm):
        self._call("handle_watermark", wm)

    def process_batch_device(self, side, dptrs, n_rows):
        """Device-resident ingest (GPU-only extension): dptrs are raw device
        addresses of the same [key, vals..., ts] columns process_batch
        takes.  Matches accumulate on the device until collect()."""
        self._call("process_batch_device", side, _ptr_array(dptrs),
                   len(dptrs), n_rows)

    def collect(self):
        """Drain device-accumulated match rows to host numpy columns."""
        return self._call_out("collect")

    def expire(self):
        self._call("expire")

    def checkpoint_drain(self, side):
        return self._call_out("checkpoint_drain", side)

    def restore(self, side, cols, watermark=None):
        keep, batch = _batch_args(cols)
        self._call("restore", side, *batch,
                   1 if watermark is not None else 0,
                   watermark if watermark is not None else 0)


class UpdAggOp(_Handle):
    """One updating (non-windowed) aggregate operator behind the C ABI,
    mirroring IncrementalAggregatingFunc's ArrowOperator surface
    (crates/arroyo-worker/src/arrow/incremental_aggregator.rs)."""

    FAMILY = "updagg_"

    def process_batch(self, cols):
        self._send("process_batch", cols)

    def process_batch_device(self, dptrs, n_rows):
        """Device-resident ingest (GPU-only extension): dptrs are raw
        device addresses of the [keys..., vals..., is_retract] columns."""
        self._call("process_batch_device", _ptr_array(dptrs), len(dptrs),
                   n_rows)

    def process_batch_nullable(self, cols, valid):
        """Nullable ingest (GPU-only extension; the C oracle has no NULLs).
        cols as for process_batch; valid is None (everything valid) or a
        list parallel to cols whose entries are None (column all valid) or
        a bool array (True = non-null)."""
        keep, (arr, n_cols, n_rows) = _batch_args(cols)
        vkeep, varr = _validity_args(valid, n_cols, n_rows)
        self._call("process_batch_nullable", arr, varr, n_cols, n_rows)

    def process_batch_nullable_device(self, dptrs, dvalid_ptrs, n_rows):
        """Device-resident nullable ingest: dptrs as for
        process_batch_device; dvalid_ptrs is None or a list parallel to
        dptrs of None / raw device addresses of Arrow validity bitmaps
        (8-byte aligned, padded to a multiple of 8 bytes)."""
        varr = None
        if dvalid_ptrs is not None:
            if len(dvalid_ptrs) != len(dptrs):
                raise ValueError(
                    f"dvalid_ptrs has {len(dvalid_ptrs)} entries for "
                    f"{len(dptrs)} cols")
            varr = _ptr_array(dvalid_ptrs)
        self._call("process_batch_nullable_device", _ptr_array(dptrs), varr,
                   len(dptrs), n_rows)

    def flush(self):
        return self._call_out("flush")

    def flush_with_validity(self):
        """flush() plus the per-column validity as bool masks (all True for
        a column without a bitmap): returns (cols, masks)."""
        return self._call_out("flush", with_validity=True)

    def expire(self, idle_flushes):
        return self._call_out("expire", idle_flushes)

    def expire_with_validity(self, idle_flushes):
        return self._call_out("expire", idle_flushes, with_validity=True)

    def checkpoint_drain(self, which):
        return self._call_out("checkpoint_drain", which)

    def restore(self, which, cols):
        self._send("restore", cols, which)


class WindowFnOp(_Handle):
    """One window-function operator behind the C ABI, mirroring
    WindowFunctionOperator's ArrowOperator surface
    (crates/arroyo-worker/src/arrow/window_fn.rs)."""

    FAMILY = "windowfn_"

    def __init__(self, lib, prefix, cfg):
        if cfg.fn != WFN_ROW_NUMBER and prefix != "arroyo_amd_":
            raise ValueError(
                f"window function {cfg.fn}: the oracle implements "
                "ROW_NUMBER only")
        super().__init__(lib, prefix, cfg)

    def handle_watermark_with_validity(self, wm):
        """handle_watermark plus the per-column validity as bool masks (all
        True for a column without a bitmap): returns (cols, masks).  Only
        the function column of LAG/LEAD without a default holds NULLs."""
        return self._call_out("handle_watermark", wm, with_validity=True)

    def process_batch(self, cols):
        self._send("process_batch", cols)

    def process_batch_device(self, dptrs, n_rows):
        """Device-resident ingest (GPU-only extension): dptrs are raw
        device addresses of the same columns process_batch takes."""
        self._call("process_batch_device", _ptr_array(dptrs), len(dptrs),
                   n_rows)

    def handle_watermark(self, wm):
        return self._call_out("handle_watermark", wm)

    def checkpoint_drain(self):
        return self._call_out("checkpoint_drain")

    def restore(self, cols):
        """Replays the drained rows through process_batch."""
        if cols and len(cols[0]):
            self.process_batch(cols)


class MapOp(_Handle):
    """One stateless map/filter/projection operator behind the C ABI,
    mirroring the expression operators' ArrowOperator surface
    (crates/arroyo-worker/src/arrow/mod.rs:48-243)."""

    FAMILY = "map_"

    def process_batch_device(self, dptrs, n_rows):
        """Device-resident map/filter (GPU-only extension): input device
        addresses in, (device output addresses, surviving row count) out.
        The returned addresses are owned by the operator and valid until
        the next process_batch* call."""
        outp = (ctypes.c_void_p * self.cfg.n_out)()
        n_out = ctypes.c_int64(0)
        self._call("process_batch_device", _ptr_array(dptrs), len(dptrs),
                   n_rows, outp, ctypes.byref(n_out))
        return [outp[i] for i in range(self.cfg.n_out)], int(n_out.value)

    def process_batch(self, cols):
        keep, batch = _batch_args(cols)
        return self._call_out("process_batch", *batch)

    def process_batch_nullable(self, cols, valid):
        """SQL NULLs in and out (GPU-only extension, null_semantics=1
        handles).  cols as for process_batch; valid is None (everything
        valid) or a list parallel to cols whose entries are None (column all
        valid) or a bool array (True = non-null).  Returns (cols, masks):
        masks[i] is output column i's validity as a bool array, all True
        for a column that came back without a bitmap; the value under a
        NULL is 0."""
        keep, (arr, n_cols, n_rows) = _batch_args(cols)
        vkeep, varr = _validity_args(valid, n_cols, n_rows)
        return self._call_out("process_batch_nullable", arr, varr, n_cols,
                              n_rows, with_validity=True)

    def process_batch_with_validity(self, cols):
        """process_batch on a null_semantics=1 handle: every input valid,
        (cols, masks) out as from process_batch_nullable."""
        keep, batch = _batch_args(cols)
        return self._call_out("process_batch", *batch, with_validity=True)

    def process_batch_nullable_device(self, dptrs, dvalid_ptrs, n_rows):
        """Device-resident counterpart: dptrs as for process_batch_device;
        dvalid_ptrs is None or a list parallel to dptrs of None / raw device
        addresses of Arrow validity bitmaps (8-byte aligned, padded to a
        multiple of 8 bytes).  Returns (output column addresses, output
        bitmap addresses, NULL count per output column, surviving rows);
        the addresses are owned by the operator and valid until the next
        process_batch* call, the bitmaps 8-byte aligned and padded to 8
        bytes with the padding bits clear."""
        varr = None
        if dvalid_ptrs is not None:
            if len(dvalid_ptrs) != len(dptrs):
                raise ValueError(
                    f"dvalid_ptrs has {len(dvalid_ptrs)} entries for "
                    f"{len(dptrs)} cols")
            varr = _ptr_array(dvalid_ptrs)
        n = self.cfg.n_out
        outp, outv = (ctypes.c_void_p * n)(), (ctypes.c_void_p * n)()
        nulls = (ctypes.c_int64 * n)()
        n_out = ctypes.c_int64(0)
        self._call("process_batch_nullable_device", _ptr_array(dptrs), varr,
                   len(dptrs), n_rows, outp, outv, nulls,
                   ctypes.byref(n_out))
        return ([outp[i] for i in range(n)], [outv[i] for i in range(n)],
                [int(nulls[i]) for i in range(n)], int(n_out.value))


# ---- Arrow Utf8 helpers and the string-key dictionary ------------------------

def strings_to_arrow(strings):
    """list[bytes | str] -> (int32 offsets [n + 1], uint8 data): the two
    buffers of an Arrow Utf8 array.  str items are encoded as UTF-8."""
    raw = [s.encode("utf-8") if isinstance(s, str) else bytes(s)
           for s in strings]
    lens = np.fromiter((len(b) for b in raw), dtype=np.int64, count=len(raw))
    offsets = np.zeros(len(raw) + 1, dtype=np.int64)
    np.cumsum(lens, out=offsets[1:])
    if offsets[-1] > np.iinfo(np.int32).max:
        raise ValueError("strings exceed the int32 offset range of Utf8")
    data = np.frombuffer(b"".join(raw), dtype=np.uint8).copy()
    return offsets.astype(np.int32), data


def arrow_to_strings(offsets, data):
    """(offsets, data) -> list[bytes]; honours a non-zero offsets[0]."""
    buf = np.ascontiguousarray(data, dtype=np.uint8).tobytes()
    off = [int(o) for o in offsets]
    return [buf[off[i]:off[i + 1]] for i in range(len(off) - 1)]


def _strbatch_to_numpy(out):
    n = int(out.n_rows)
    ids = np.ctypeslib.as_array(out.ids, shape=(n,)).copy() if n else \
        np.zeros(0, dtype=np.int64)
    offsets = np.ctypeslib.as_array(out.offsets, shape=(n + 1,)).copy()
    total = int(offsets[-1])
    data = np.ctypeslib.as_array(out.data, shape=(total,)).copy() if total \
        else np.zeros(0, dtype=np.uint8)
    return ids, offsets, data


class StrKeyDict(_Handle):
    """Device-resident string interner behind the C ABI: Arrow Utf8 key
    columns in, stable non-negative int64 ids out (and back).  Share one
    instance between every operator that must agree on the ids."""

    FAMILY = "strkey_"

    @staticmethod
    def _arrow(offsets, data):
        offsets = np.ascontiguousarray(offsets, dtype=np.int32)
        data = np.ascontiguousarray(data, dtype=np.uint8)
        if len(offsets) < 1:
            raise ValueError("offsets needs n_rows + 1 entries")
        return offsets, data

    def _call_strs(self, name, *args):
        """Call a function whose last parameter is an AmdStrBatch*; return
        (ids, offsets, data) and free the batch."""
        out = AmdStrBatch()
        self._call(name, *args, ctypes.byref(out))
        res = _strbatch_to_numpy(out)
        self._fn["free_out"](ctypes.byref(out))
        return res

    def encode(self, offsets, data, with_hashes=False):
        """Host Arrow buffers -> int64 ids (and uint64 content hashes when
        with_hashes)."""
        offsets, data = self._arrow(offsets, data)
        n = len(offsets) - 1
        ids = np.empty(n, dtype=np.int64)
        hashes = np.empty(n, dtype=np.uint64) if with_hashes else None
        self._call("encode", offsets.ctypes.data, data.ctypes.data, n,
                   ids.ctypes.data,
                   hashes.ctypes.data if with_hashes else None)
        return (ids, hashes) if with_hashes else ids

    def encode_device(self, d_offsets, d_data, n, d_ids, d_hashes=None):
        """Device pointers (ints) in, ids (and hashes) written on device;
        synchronised on return."""
        self._call("encode_device", d_offsets, d_data, n, d_ids, d_hashes)

    def decode(self, ids):
        """int64 ids -> (int32 offsets, uint8 data)."""
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        _, offsets, data = self._call_strs("decode", ids.ctypes.data,
                                           len(ids))
        return offsets, data

    def drain(self):
        """Checkpoint: every interned string -> (ids, offsets, data)."""
        return self._call_strs("checkpoint_drain")

    def restore(self, ids, offsets, data):
        """Load a drain() into this (empty) handle; every string keeps its
        id."""
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        offsets, data = self._arrow(offsets, data)
        if len(ids) != len(offsets) - 1:
            raise ValueError("ids and offsets disagree on the row count")
        self._call("restore", ids.ctypes.data, offsets.ctypes.data,
                   data.ctypes.data, len(ids))

    def count(self):
        """Number of interned strings."""
        n = ctypes.c_int64(0)
        self._call("count", ctypes.byref(n), None)
        return int(n.value)

    def profile(self, enable=None):
        """Switch per-encode timing of the lookup kernel on/off (None leaves
        it); returns the kernel milliseconds of the last timed encode."""
        ms = ctypes.c_double(0.0)
        self._call("profile", -1 if enable is None else int(bool(enable)),
                   ctypes.byref(ms))
        return ms.value

    def arena_used(self):
        """Arena bytes in use (each string rounded up to 8 bytes)."""
        used = ctypes.c_int64(0)
        self._call("count", None, ctypes.byref(used))
        return int(used.value)


# ---- the tuple-key dictionary ------------------------------------------------

def _words(col):
    """An 8-byte column (i64, u64, f64) as the contiguous int64 view of its
    raw bits."""
    col = np.ascontiguousarray(col)
    if col.dtype.itemsize != 8 or col.ndim != 1:
        raise ValueError("tuple components are 1-D columns of 8-byte elements")
    return col.view(np.int64)


def _out_masks(out):
    """The validity of an AmdOutBatch as it stands: None when the batch has
    no validity table, else a list with None for a column without a bitmap
    and a bool mask (True = non-null) otherwise."""
    return out_validity(out) if out.validity else None


class TupleKeyDict(_Handle):
    """Device-resident interner for composite and nullable keys behind the
    C ABI: tuples of up to 8 64-bit words, each optionally NULL, in; stable
    non-negative int64 ids out (and back).  Share one instance between every
    operator that must agree on the ids."""

    FAMILY = "tuplekey_"

    def _host_batch(self, cols, valid):
        """(arrays to hold, column table, bitmap table, rows) of a host
        batch.  valid is None or a list parallel to cols of None (column all
        valid), a bool mask (True = non-null) or an already packed Arrow
        bitmap (uint8, at least (rows + 7) // 8 bytes)."""
        if len(cols) != self.cfg.n_cols:
            raise ValueError(
                f"{len(cols)} columns for a handle of {self.cfg.n_cols}")
        keep = [_words(c) for c in cols]
        n = len(keep[0])
        if any(len(c) != n for c in keep):
            raise ValueError("columns differ in length")
        varr = None
        if valid is not None:
            if len(valid) != len(cols):
                raise ValueError(
                    f"valid has {len(valid)} entries for {len(cols)} cols")
            ptrs = []
            for m in valid:
                if m is None:
                    ptrs.append(None)
                    continue
                m = np.asarray(m)
                if m.dtype == np.uint8:
                    bm = np.ascontiguousarray(m)
                    if len(bm) < (n + 7) // 8:
                        raise ValueError("packed bitmap shorter than "
                                         "(n_rows + 7) // 8 bytes")
                else:
                    if len(m) != n:
                        raise ValueError("validity mask length != n_rows")
                    bm = pack_validity(m)
                if len(bm) == 0:
                    bm = np.zeros(1, dtype=np.uint8)
                keep.append(bm)
                ptrs.append(bm.ctypes.data)
            varr = _ptr_array(ptrs)
        return keep, _ptr_array([c.ctypes.data for c in keep[:len(cols)]]), \
            varr, n

    def _call_tuples(self, name, *args):
        """Call a function whose last parameter is an AmdOutBatch*; return
        (cols, masks) with masks as _out_masks gives them."""
        out = AmdOutBatch()
        self._call(name, *args, ctypes.byref(out))
        cols, masks = _out_to_numpy(out), _out_masks(out)
        self._fn["free_out"](ctypes.byref(out))
        return cols, masks

    def encode(self, cols, valid=None, want_hashes=False):
        """Host columns (and validity) -> int64 ids (and uint64 content
        hashes when want_hashes)."""
        keep, carr, varr, n = self._host_batch(cols, valid)
        ids = np.empty(n, dtype=np.int64)
        hashes = np.empty(n, dtype=np.uint64) if want_hashes else None
        self._call("encode", carr, varr, n, ids.ctypes.data,
                   hashes.ctypes.data if want_hashes else None)
        return (ids, hashes) if want_hashes else ids

    @staticmethod
    def _dev_tables(d_cols, d_valid):
        if d_valid is not None and len(d_valid) != len(d_cols):
            raise ValueError(
                f"d_valid has {len(d_valid)} entries for {len(d_cols)} cols")
        return _ptr_array(d_cols), \
            None if d_valid is None else _ptr_array(d_valid)

    def encode_device(self, d_cols, d_valid, n, d_ids, d_hashes=None):
        """Device addresses (ints) in: d_cols one per component, d_valid
        None or a list of None / addresses of 8-byte aligned bitmaps padded
        to 8 bytes.  Ids (and hashes) are written on the device;
        synchronised on return."""
        carr, varr = self._dev_tables(d_cols, d_valid)
        self._call("encode_device", carr, varr, n, d_ids, d_hashes)

    def hash_device(self, d_cols, d_valid, n, d_hashes):
        """The content hash alone; touches no table state."""
        carr, varr = self._dev_tables(d_cols, d_valid)
        self._call("hash_device", carr, varr, n, d_hashes)

    def decode(self, ids):
        """int64 ids -> (cols, masks): n_cols int64 columns of raw words (0
        under a NULL); masks is None when no decoded component is NULL, else
        a list with a bool mask (True = non-null) for exactly the columns
        that hold one and None for the others."""
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        return self._call_tuples("decode", ids.ctypes.data, len(ids))

    def decode_device(self, d_ids, n, d_cols_out, d_valid_out=None):
        """Device ids -> device columns and, on a nullable handle, validity
        words ((n + 63) // 64 uint64 per column, written in full)."""
        carr, varr = self._dev_tables(d_cols_out, d_valid_out)
        self._call("decode_device", d_ids, n, carr, varr)

    def count(self):
        """Number of interned tuples."""
        n = ctypes.c_int64(0)
        self._call("count", ctypes.byref(n))
        return int(n.value)

    def drain(self):
        """Checkpoint: every interned tuple -> (ids, cols, masks), cols and
        masks as decode returns them."""
        cols, masks = self._call_tuples("checkpoint_drain")
        return cols[0], cols[1:], None if masks is None else masks[1:]

    def restore(self, ids, cols, valid=None):
        """Load a drain() into this (empty) handle; every tuple keeps its
        id."""
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        keep, carr, varr, n = self._host_batch(cols, valid)
        if len(ids) != n:
            raise ValueError("ids and cols disagree on the row count")
        self._call("restore", ids.ctypes.data, carr, varr, n)
