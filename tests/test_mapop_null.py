"""SQL NULLs through the map operator (AmdMapConfig.null_semantics = 1).

`ref_eval` below is an independent reference written from the rules in
include/arroyo_amd_types.h (restated from arrow-arith / DataFusion, not
golden-pinned): numpy over (value, valid) pairs, one array pair per
register.  It shares no code with the kernel.  Wrapping arithmetic goes
through uint64; division and remainder are built from the C remainder
(np.fmod) and checked against hand-worked literals below.

Comparison is bit-exact on values where valid (an f64 NaN only has to be a
NaN), exact on validity, and exactly 0 under a NULL.  The CPU oracle has no
NULLs: its loud rejection of null_semantics = 1 is pinned here too."""
import ctypes
import functools
import math

import numpy as np
import pytest

import oracle
from arroyo_amd import cabi
from arroyo_amd.cabi import (MOP_ADD, MOP_AND, MOP_COALESCE, MOP_CONST,
                             MOP_DIV, MOP_EQ, MOP_F2I, MOP_FADD, MOP_FDIV,
                             MOP_FMUL, MOP_FSUB, MOP_GE, MOP_GT, MOP_I2F,
                             MOP_IS_NOT_NULL, MOP_IS_NULL, MOP_LE, MOP_LT,
                             MOP_MOD, MOP_MUL, MOP_NE, MOP_NOT, MOP_NULLIF,
                             MOP_OR, MOP_SELECT, MOP_SUB)
# the edge values and the device-buffer helper of the opcode suite
from test_mapop_ops import (EF_BITS, EF_CASTABLE, EI, FLOAT_CONSTS, Hip, b2f,
                            f2b, gen_inputs)

I64_MIN, I64_MAX = -2**63, 2**63 - 1
MAX_PROG, MAX_REGS = 64, 32
GARBAGE = I64_MIN           # what lies under an input NULL
CHUNK = 1 << 20             # rows the host surface stages per launch


# ------------------------------------------------------------ the reference

def _u(x):
    return x.view(np.uint64)


def _i(x):
    return x.view(np.int64)


class _Rows:
    """Row errors of one batch.  A row that raised stops there: it raises
    nothing further."""

    def __init__(self, n):
        self.alive = np.ones(n, dtype=bool)
        self.kinds = set()

    def throw(self, kind, rows):
        rows = rows & self.alive
        if rows.any():
            self.kinds.add(kind)
            self.alive &= ~rows


def _step(op, a, b, c, imm, n, rows):
    """One instruction over all rows: a, b, c are (value, valid) pairs (c is
    SELECT's else-register).  Returns the result pair; the value under a
    NULL is whatever falls out, the caller zeroes it."""
    (va, oa), (vb, ob) = a, b
    yes = np.ones(n, dtype=bool)
    if op == MOP_CONST:
        bits = f2b(imm) if isinstance(imm, float) else imm
        return np.full(n, bits, dtype=np.int64), yes
    if op == MOP_IS_NULL:
        return (~oa).astype(np.int64), yes
    if op == MOP_IS_NOT_NULL:
        return oa.astype(np.int64), yes
    if op == MOP_COALESCE:
        return np.where(oa, va, vb), oa | ob
    if op == MOP_NULLIF:
        return va, oa & ~(ob & (va == vb))
    if op == MOP_SELECT:
        vc, oc = c
        cond = oa & (va != 0)
        return np.where(cond, vb, vc), np.where(cond, ob, oc)
    if op == MOP_AND:
        false = (oa & (va == 0)) | (ob & (vb == 0))
        ok = false | (oa & ob)
        return (ok & ~false).astype(np.int64), ok
    if op == MOP_OR:
        true = (oa & (va != 0)) | (ob & (vb != 0))
        return true.astype(np.int64), true | (oa & ob)
    if op == MOP_NOT:
        return (va == 0).astype(np.int64), oa
    if op == MOP_I2F:
        return _i(va.astype(np.float64)), oa        # int -> float rounds RNE
    if op == MOP_F2I:
        x = va.view(np.float64)
        fits = np.isfinite(x) & (x >= -2.0**63) & (x < 2.0**63)
        rows.throw("cast", oa & ~fits)              # valid slots only
        return np.trunc(np.where(fits, x, 0.0)).astype(np.int64), oa
    ok = oa & ob                                    # binary: propagation
    if op in (MOP_DIV, MOP_MOD):
        rows.throw("division by zero", ok & (vb == 0))
        if op == MOP_DIV:
            rows.throw("overflow", ok & (va == I64_MIN) & (vb == -1))
        plain = ok & (vb != 0) & (vb != -1)
        d = np.where(plain, vb, 1)
        r = np.fmod(va, d)                          # sign of the dividend
        if op == MOP_MOD:
            return np.where(plain, r, 0), ok        # x % -1 == 0
        q = (va - r) // d                           # exact, so truncated
        return np.where(vb == -1, _i(0 - _u(va)), q), ok
    if op >= MOP_FADD:
        x, y = va.view(np.float64), vb.view(np.float64)
        with np.errstate(all="ignore"):
            z = {MOP_FADD: np.add, MOP_FSUB: np.subtract,
                 MOP_FMUL: np.multiply, MOP_FDIV: np.divide}[op](x, y)
        return _i(z), ok
    if op in (MOP_ADD, MOP_SUB, MOP_MUL):
        f = {MOP_ADD: np.add, MOP_SUB: np.subtract, MOP_MUL: np.multiply}[op]
        return _i(f(_u(va), _u(vb))), ok
    cmp = {MOP_EQ: np.equal, MOP_NE: np.not_equal, MOP_LT: np.less,
           MOP_LE: np.less_equal, MOP_GT: np.greater,
           MOP_GE: np.greater_equal}[op]
    return cmp(va, vb).astype(np.int64), ok


def ref_eval(cfg, cols, valid=None):
    """cfg = (n_in_cols, prog, out_reg, filter_reg); cols = int64 columns;
    valid = None or per column None / bool array.  Returns (values, masks)
    of the emitted rows, values exactly 0 under a NULL, or the kind of error
    the batch raises.  A register holds nothing before it is written (a
    KeyError here)."""
    n_in, prog, out_reg, filter_reg = cfg
    assert len(cols) == n_in
    n = len(cols[0])
    valid = valid or [None] * n_in
    regs = {}
    for i, (col, ok) in enumerate(zip(cols, valid)):
        ok = np.ones(n, dtype=bool) if ok is None else np.asarray(ok, bool)
        regs[i] = (np.where(ok, np.asarray(col, dtype=np.int64), 0), ok)
    rows = _Rows(n)
    for ins in prog:
        op, a, b, dst = ins[:4]
        imm = ins[4] if len(ins) > 4 else 0
        # CONST reads nothing: its operand fields may name unwritten registers
        ra, rb = (regs[0], regs[0]) if op == MOP_CONST else \
            (regs[a], regs[a] if op in (MOP_NOT, MOP_I2F, MOP_F2I,
                                        MOP_IS_NULL, MOP_IS_NOT_NULL)
             else regs[b])
        rc = regs[imm] if op == MOP_SELECT else None
        v, ok = _step(op, ra, rb, rc, imm, n, rows)
        ok = np.asarray(ok, dtype=bool)
        regs[dst] = (np.where(ok, v, 0).astype(np.int64), ok)
    # which error a batch of mixed errors reports is unspecified
    assert len(rows.kinds) <= 1, f"test batch mixes error kinds: {rows.kinds}"
    if rows.kinds:
        return rows.kinds.pop()
    keep = np.ones(n, dtype=bool)
    if filter_reg >= 0:
        v, ok = regs[filter_reg]
        keep = ok & (v != 0)                        # NULL predicate: dropped
    return ([regs[r][0][keep] for r in out_reg],
            [regs[r][1][keep] for r in out_reg])


def _one(op, a, b=(0, True), c=(0, True)):
    """op over one row of (value, valid) operands -> (value, valid) or the
    error kind; None stands for NULL in the result."""
    prog = [(op, 0, 1, 3, 2)] if op == MOP_SELECT else [(op, 0, 1, 3)]
    out = ref_eval((3, prog, [3], -1),
                   [np.array([x[0]], dtype=np.int64) for x in (a, b, c)],
                   [np.array([x[1]]) for x in (a, b, c)])
    if isinstance(out, str):
        return out
    assert out[1][0][0] or out[0][0][0] == 0
    return int(out[0][0][0]) if out[1][0][0] else None


NULL = (GARBAGE, False)


def V(x):
    return (x, True)


def test_reference_literals():
    """The reference itself, against results worked out by hand."""
    T, F = V(1), V(0)
    kleene_and = {(T, T): 1, (T, F): 0, (F, T): 0, (F, F): 0,
                  (T, NULL): None, (NULL, T): None, (F, NULL): 0,
                  (NULL, F): 0, (NULL, NULL): None}
    kleene_or = {(T, T): 1, (T, F): 1, (F, T): 1, (F, F): 0,
                 (T, NULL): 1, (NULL, T): 1, (F, NULL): None,
                 (NULL, F): None, (NULL, NULL): None}
    for (a, b), want in kleene_and.items():
        assert _one(MOP_AND, a, b) == want, ("AND", a, b)
    for (a, b), want in kleene_or.items():
        assert _one(MOP_OR, a, b) == want, ("OR", a, b)
    assert _one(MOP_AND, V(-5), V(I64_MIN)) == 1      # truthiness is != 0
    assert _one(MOP_NOT, NULL) is None and _one(MOP_NOT, V(0)) == 1
    # IS NULL / IS NOT NULL are never NULL
    assert _one(MOP_IS_NULL, NULL) == 1 and _one(MOP_IS_NULL, V(0)) == 0
    assert _one(MOP_IS_NOT_NULL, NULL) == 0
    assert _one(MOP_IS_NOT_NULL, V(I64_MIN)) == 1
    # COALESCE
    assert _one(MOP_COALESCE, V(7), V(8)) == 7
    assert _one(MOP_COALESCE, V(7), NULL) == 7
    assert _one(MOP_COALESCE, NULL, V(8)) == 8
    assert _one(MOP_COALESCE, NULL, NULL) is None
    assert _one(MOP_COALESCE, V(0), V(8)) == 0        # a valid 0 is a value
    # NULLIF
    assert _one(MOP_NULLIF, V(7), V(7)) is None
    assert _one(MOP_NULLIF, V(7), V(8)) == 7
    assert _one(MOP_NULLIF, V(7), NULL) == 7
    assert _one(MOP_NULLIF, NULL, V(7)) is None
    assert _one(MOP_NULLIF, NULL, NULL) is None
    assert _one(MOP_NULLIF, V(GARBAGE), NULL) == GARBAGE  # not the garbage
    # SELECT: CASE WHEN a THEN b ELSE c END
    assert _one(MOP_SELECT, V(1), V(5), V(6)) == 5
    assert _one(MOP_SELECT, V(-9), V(5), V(6)) == 5
    assert _one(MOP_SELECT, V(0), V(5), V(6)) == 6
    assert _one(MOP_SELECT, NULL, V(5), V(6)) == 6    # NULL is not true
    assert _one(MOP_SELECT, V(1), NULL, V(6)) is None
    assert _one(MOP_SELECT, V(0), V(5), NULL) is None
    assert _one(MOP_SELECT, V(1), V(5), NULL) == 5
    assert _one(MOP_SELECT, NULL, NULL, V(6)) == 6
    # propagation, and no error where the result is NULL
    assert _one(MOP_ADD, V(I64_MAX), V(1)) == I64_MIN
    assert _one(MOP_ADD, V(1), NULL) is None
    assert _one(MOP_EQ, NULL, NULL) is None
    assert _one(MOP_DIV, V(1), V(0)) == "division by zero"
    assert _one(MOP_MOD, V(1), V(0)) == "division by zero"
    assert _one(MOP_DIV, NULL, V(0)) is None
    assert _one(MOP_MOD, NULL, V(0)) is None
    assert _one(MOP_DIV, V(1), (0, False)) is None
    assert _one(MOP_DIV, V(I64_MIN), V(-1)) == "overflow"
    assert _one(MOP_DIV, (I64_MIN, False), V(-1)) is None
    assert _one(MOP_F2I, V(f2b(math.nan))) == "cast"
    assert _one(MOP_F2I, (f2b(math.nan), False)) is None
    assert _one(MOP_I2F, NULL) is None
    assert _one(MOP_FADD, V(f2b(1.5)), NULL) is None
    assert _one(MOP_FADD, V(f2b(1.5)), V(f2b(0.25))) == f2b(1.75)
    # the arithmetic the NULL rules sit on
    assert _one(MOP_DIV, V(-7), V(2)) == -3 and _one(MOP_DIV, V(7), V(-2)) == -3
    assert _one(MOP_MOD, V(-7), V(2)) == -1 and _one(MOP_MOD, V(7), V(-2)) == 1
    assert _one(MOP_MOD, V(I64_MIN), V(-1)) == 0
    assert _one(MOP_DIV, V(I64_MAX), V(-1)) == -I64_MAX
    assert _one(MOP_DIV, V(I64_MIN), V(2)) == -2**62
    assert _one(MOP_MUL, V(I64_MIN), V(-1)) == I64_MIN
    assert _one(MOP_F2I, V(f2b(-1.5))) == -1
    assert _one(MOP_I2F, V(2**53 + 1)) == f2b(2.0**53)
    # a CONST is always valid, and a NULL predicate drops the row
    out = ref_eval((1, [(MOP_CONST, 0, 0, 1, 4)], [1, 0], 0),
                   [np.array([1, 1, 0, 5])],
                   [np.array([True, False, True, True])])
    assert out[0][0].tolist() == [4, 4] and out[0][1].tolist() == [1, 5]
    assert all(m.all() for m in out[1])
    # the guarded division: SELECT(b != 0, a / NULLIF(b, 0), -1)
    guarded = [(MOP_CONST, 0, 0, 2, 0), (MOP_NE, 1, 2, 3),
               (MOP_NULLIF, 1, 2, 4), (MOP_DIV, 0, 4, 5),
               (MOP_CONST, 0, 0, 6, -1), (MOP_SELECT, 3, 5, 7, 6)]
    out = ref_eval((2, guarded, [7], -1),
                   [np.array([7, 7, 7]), np.array([2, 0, 0])],
                   [None, np.array([True, True, False])])
    assert out[0][0].tolist() == [3, -1, -1] and out[1][0].all()


# --------------------------------------------------------------- the harness

def make_cfg(cfg, out_is_f64=None, ns=1):
    n_in, prog, out_reg, filter_reg = cfg
    return cabi.make_map_config(n_in_cols=n_in, prog=prog, out_reg=out_reg,
                                out_is_f64=out_is_f64, filter_reg=filter_reg,
                                null_semantics=ns)


def i64_cols(cols):
    return [np.ascontiguousarray(c, dtype=np.int64) for c in cols]


def error_kind(exc):
    msg = str(exc)
    for kind in ("division by zero", "overflow", "cast"):
        if kind in msg:
            return kind
    raise exc


def run(cfg, cols, valid, out_is_f64=None):
    """The HIP operator's (values, masks), or the kind of error it raised."""
    from arroyo_amd import gpu
    op = gpu.make_map_op(make_cfg(cfg, out_is_f64))
    try:
        return op.process_batch_nullable(i64_cols(cols), valid)
    except RuntimeError as e:
        return error_kind(e)
    finally:
        op.close()


def assert_result(got, want, out_is_f64=None):
    assert not isinstance(got, str), f"raised {got!r}"
    (gc, gm), (wc, wm) = got, want
    assert len(gc) == len(wc) == len(gm) == len(wm)
    for i, (g, m, w, k) in enumerate(zip(gc, gm, wc, wm)):
        f = bool(out_is_f64 and out_is_f64[i])
        assert g.dtype == (np.float64 if f else np.int64)
        gb, wb = g.view(np.int64), np.asarray(w, dtype=np.int64)
        assert gb.shape == wb.shape, (i, gb.shape, wb.shape)
        assert np.array_equal(m, k), (i, np.flatnonzero(m != k)[:5])
        assert not gb[~k].any(), (i, "value under a NULL is not 0")
        if f:
            nan = k & np.isnan(wb.view(np.float64))
            assert np.array_equal(k & np.isnan(g), nan)
            k = k & ~nan
        bad = np.flatnonzero(k & (gb != wb))
        assert bad.size == 0, (i, bad[:5], gb[bad[:5]], wb[bad[:5]])


def check(cfg, cols, valid, out_is_f64=None, want=None):
    want = ref_eval(cfg, i64_cols(cols), valid) if want is None else want
    got = run(cfg, cols, valid, out_is_f64)
    if isinstance(want, str):
        assert isinstance(got, str), f"no error, want {want!r}"
        assert got == want
    else:
        assert_result(got, want, out_is_f64)
    return want


def raw_batch(op, fn, cols, bitmaps=None):
    """Call a host entry point on already packed bitmaps (None, or per
    column None / uint8 array) and return (cols, masks, has_table): masks[i]
    is None for a column that came back without a bitmap, has_table says
    whether out->validity itself was set."""
    keep, (arr, n_cols, n_rows) = cabi._batch_args(i64_cols(cols))
    out = cabi.AmdOutBatch()
    if fn == "process_batch":
        args = (arr, n_cols, n_rows)
    else:
        varr = None
        if bitmaps is not None:
            varr = cabi._ptr_array([None if b is None else b.ctypes.data
                                    for b in bitmaps])
        args = (arr, varr, n_cols, n_rows)
    op._call(fn, *args, ctypes.byref(out))
    got = cabi._out_to_numpy(out)
    masks = cabi.out_validity(out)
    has_table = bool(out.validity)
    # padding bits of every returned bitmap are clear
    for i in range(out.n_cols):
        if has_table and out.validity[i] and out.n_rows % 8:
            last = out.validity[i][(out.n_rows - 1) // 8]
            assert last >> (out.n_rows % 8) == 0, "padding bits set"
    op._fn["free_out"](ctypes.byref(out))
    return got, masks, has_table


def dirty_bitmap(mask):
    """Arrow bitmap of a bool mask with every padding bit set."""
    bm = cabi.pack_validity(mask)
    if len(mask) % 8:
        bm[-1] |= (0xFF << (len(mask) % 8)) & 0xFF
    return bm if len(bm) else np.zeros(1, dtype=np.uint8)


# ------------------------------------------- CPU: oracle, validation, mirrors

NULL_OPS = {"IS_NULL": MOP_IS_NULL, "IS_NOT_NULL": MOP_IS_NOT_NULL,
            "COALESCE": MOP_COALESCE, "NULLIF": MOP_NULLIF,
            "SELECT": MOP_SELECT}


def test_oracle_rejects_null_semantics_loudly():
    with pytest.raises(RuntimeError,
                       match="null_semantics is not supported here"):
        oracle.make_map_op(make_cfg((1, [], [0], -1), ns=1))
    oracle.make_map_op(make_cfg((1, [], [0], -1), ns=0)).close()


def hip_create_message(cfg):
    """What arroyo_amd_map_create says to cfg: None when it made a handle
    (a GPU is present), else its message.  Validation runs before the device
    is touched, so a bad config gets its validation message anywhere and a
    good one gets a handle or "no HIP device"."""
    from arroyo_amd import gpu
    fn = cabi._family_fns(gpu.lib(), "arroyo_amd_", "map_")
    h = fn["create"](ctypes.byref(cfg))
    if h:
        fn["destroy"](h)
        return None
    return fn["last_error"](None).decode()


def assert_accepted(cfg):
    msg = hip_create_message(cfg)
    assert msg is None or "no HIP device" in msg, msg


@pytest.mark.parametrize("name", NULL_OPS)
def test_hip_validation_null_opcodes_need_null_semantics(name):
    prog = [(NULL_OPS[name], 0, 1, 2, 0)]
    bad = hip_create_message(make_cfg((2, prog, [2], -1), ns=0))
    assert bad is not None and "unknown opcode" in bad, bad
    assert_accepted(make_cfg((2, prog, [2], -1), ns=1))


def test_hip_validation_select_else_register():
    def select(imm):
        return make_cfg((2, [(MOP_SELECT, 0, 1, 2, imm)], [2], -1))
    for imm in (-1, MAX_REGS, 2**31, 2**40 + 1):
        msg = hip_create_message(select(imm))
        assert msg is not None and "out of range" in msg, (imm, msg)
    for imm in (2, 5, MAX_REGS - 1):            # in range, never written
        msg = hip_create_message(select(imm))
        assert msg is not None and "read before it is written" in msg, msg
    assert_accepted(select(0))
    assert_accepted(select(1))
    # written by an earlier instruction: fine; by a later one: not
    k = (MOP_CONST, 0, 0, 9, 4)
    assert_accepted(make_cfg((2, [k, (MOP_SELECT, 0, 1, 2, 9)], [2], -1)))
    msg = hip_create_message(
        make_cfg((2, [(MOP_SELECT, 0, 1, 2, 9), k], [2], -1)))
    assert msg is not None and "read before it is written" in msg, msg


def test_hip_validation_read_sets_of_null_opcodes():
    # IS_NULL / IS_NOT_NULL read a only: b may name an unwritten register
    for op in (MOP_IS_NULL, MOP_IS_NOT_NULL):
        assert_accepted(make_cfg((1, [(op, 0, 7, 1)], [1], -1)))
        msg = hip_create_message(make_cfg((1, [(op, 7, 0, 1)], [1], -1)))
        assert msg is not None and "read before it is written" in msg, msg
    # COALESCE / NULLIF / SELECT read a and b
    for op in (MOP_COALESCE, MOP_NULLIF, MOP_SELECT):
        for a, b in ((7, 0), (0, 7)):
            msg = hip_create_message(
                make_cfg((1, [(op, a, b, 1, 0)], [1], -1)))
            assert msg is not None and "read before it is written" in msg


@pytest.mark.parametrize("ns", [2, -1, 256])
def test_hip_validation_null_semantics_value(ns):
    msg = hip_create_message(make_cfg((1, [], [0], -1), ns=ns))
    assert msg is not None and "null_semantics" in msg, msg
    assert_accepted(make_cfg((1, [], [0], -1), ns=1))
    assert_accepted(make_cfg((1, [], [0], -1), ns=0))


def test_config_mirror_and_prototypes():
    """The new field is the struct's last, and both entry points are in the
    prototype table with the header's parameter counts and exported."""
    from arroyo_amd import gpu
    fields = [f[0] for f in cabi.AmdMapConfig._fields_]
    assert fields[-1] == "null_semantics" and fields[-2] == "emit_to_host"
    assert make_cfg((1, [], [0], -1), ns=0).null_semantics == 0
    assert cabi.make_map_config(1, [], [0]).null_semantics == 0
    assert (cabi.MOP_IS_NULL, cabi.MOP_IS_NOT_NULL, cabi.MOP_COALESCE,
            cabi.MOP_NULLIF, cabi.MOP_SELECT) == (21, 22, 23, 24, 25)
    assert cabi.MOP_IS_NULL == cabi.MOP_FDIV + 1
    assert len(cabi.PROTOTYPES["map_process_batch_nullable"][1]) == 6
    assert len(cabi.PROTOTYPES["map_process_batch_nullable_device"][1]) == 9
    lib = gpu.lib()
    for name in ("map_process_batch_nullable",
                 "map_process_batch_nullable_device"):
        assert getattr(lib, "arroyo_amd_" + name).argtypes is not None


def test_null_opcode_constants_match_header(tmp_path):
    """What the host C compiler makes of include/arroyo_amd_map_null.h,
    reached through arroyo_amd_types.h as every user reaches it: each
    constant it defines has a Python twin of the same value, and
    AmdMapConfig is the mirror's size with null_semantics at its offset."""
    import os
    import re
    import subprocess
    inc = os.path.join(os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))), "include")
    hdr = open(os.path.join(inc, "arroyo_amd_map_null.h")).read()
    body = hdr[hdr.index("enum AmdMapNullOp"):]
    names = sorted(set(re.findall(r"\b(AMD_MOP_[A-Z_]*[A-Z])\b", body)))
    assert len(names) == 5, names
    lines = ["#include <stdio.h>", "#include <stddef.h>",
             '#include "arroyo_amd_types.h"', "int main(void) {"]
    lines += [f'printf("{n} %d\\n", (int)({n}));' for n in names]
    lines += ['printf("sizeof %zu\\n", sizeof(AmdMapConfig));',
              'printf("offset %zu\\n", '
              'offsetof(AmdMapConfig, null_semantics));', "return 0;", "}"]
    src, exe = tmp_path / "nullops.c", tmp_path / "nullops"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run(["gcc", "-std=c11", "-I", inc, "-o", str(exe), str(src)],
                   check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True,
                         text=True).stdout
    facts = {k: int(v) for k, v in (line.split() for line in out.splitlines())}
    for n in names:
        assert getattr(cabi, n[len("AMD_"):]) == facts[n], n
    assert sorted(facts[n] for n in names) == [21, 22, 23, 24, 25]
    assert facts["sizeof"] == ctypes.sizeof(cabi.AmdMapConfig)
    assert facts["offset"] == cabi.AmdMapConfig.null_semantics.offset


# ------------------------------------------------- GPU: edge grids per opcode

def with_nulls(pairs, null_divisor_zero=False):
    """Every operand pair crossed with {valid, NULL} on each side; GARBAGE
    under a NULL (0 under a NULL divisor when asked)."""
    a, b, oa, ob = [], [], [], []
    for x, y in pairs:
        for va in (True, False):
            for vb in (True, False):
                a.append(x if va else GARBAGE)
                b.append(y if vb else (0 if null_divisor_zero else GARBAGE))
                oa.append(va)
                ob.append(vb)
    return [a, b], [np.array(oa), np.array(ob)]


EI_PAIRS = [(a, b) for a in EI for b in EI]
EF_PAIRS = [(a, b) for a in EF_BITS for b in EF_BITS]

BIN_OPS = {"ADD": MOP_ADD, "SUB": MOP_SUB, "MUL": MOP_MUL, "EQ": MOP_EQ,
           "NE": MOP_NE, "LT": MOP_LT, "LE": MOP_LE, "GT": MOP_GT,
           "GE": MOP_GE, "AND": MOP_AND, "OR": MOP_OR,
           "COALESCE": MOP_COALESCE, "NULLIF": MOP_NULLIF}


def binary(op):
    return (2, [(op, 0, 1, 2)], [2], -1)


@pytest.mark.gpu
@pytest.mark.parametrize("name", BIN_OPS)
def test_int_grid_binary(name):
    cols, valid = with_nulls(EI_PAIRS)
    want = check(binary(BIN_OPS[name]), cols, valid)
    assert 0 < want[1][0].sum() < len(cols[0])      # NULLs and values


@pytest.mark.gpu
@pytest.mark.parametrize("op", [MOP_DIV, MOP_MOD], ids=["DIV", "MOD"])
def test_int_grid_divmod(op):
    """Every pair, the erroring ones included, raises nothing where an
    operand is NULL; the valid x valid rows are the non-erroring pairs."""
    ok = [(a, b) for a, b in EI_PAIRS
          if b != 0 and not (op == MOP_DIV and (a, b) == (I64_MIN, -1))]
    cols, valid = with_nulls(ok, null_divisor_zero=True)
    # the erroring pairs, with one or both operands NULL: x / 0 under a
    # valid 0 divisor needs a NULL dividend
    for a, b in ((5, 0), (I64_MIN, -1), (0, 0), (I64_MIN, 0)):
        for va, vb in ((False, True), (True, False), (False, False)):
            cols[0].append(a)
            cols[1].append(b)
            valid[0] = np.append(valid[0], va)
            valid[1] = np.append(valid[1], vb)
    want = check(binary(op), cols, valid)
    assert not isinstance(want, str)
    assert want[1][0].sum() == len(ok)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["NOT", "I2F", "IS_NULL", "IS_NOT_NULL"])
def test_int_grid_unary(name):
    op = {"NOT": MOP_NOT, "I2F": MOP_I2F, **NULL_OPS}[name]
    vals = EI + [GARBAGE] * len(EI)
    valid = [np.array([True] * len(EI) + [False] * len(EI))]
    f = [int(op == MOP_I2F)]
    # b names an unwritten register: it is not read
    want = check((1, [(op, 0, 9, 1)], [1], -1), [vals], valid, out_is_f64=f)
    if op in (MOP_IS_NULL, MOP_IS_NOT_NULL):
        assert want[1][0].all()
        assert want[0][0].tolist() == [int(op == MOP_IS_NOT_NULL)] * len(EI) \
            + [int(op == MOP_IS_NULL)] * len(EI)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["FADD", "FSUB", "FMUL", "FDIV"])
def test_float_grid(name):
    op = {"FADD": MOP_FADD, "FSUB": MOP_FSUB, "FMUL": MOP_FMUL,
          "FDIV": MOP_FDIV}[name]
    cols, valid = with_nulls(EF_PAIRS)
    check(binary(op), cols, valid, out_is_f64=[1])


@pytest.mark.gpu
def test_float_grid_f2i():
    """In-range values valid, every value -- NaN, inf and out of range
    included -- under a NULL."""
    castable = [b for b, ok in zip(EF_BITS, EF_CASTABLE) if ok]
    vals = castable + EF_BITS
    valid = [np.array([True] * len(castable) + [False] * len(EF_BITS))]
    want = check((1, [(MOP_F2I, 0, 0, 1)], [1], -1), [vals], valid)
    assert want[1][0].sum() == len(castable)


@pytest.mark.gpu
def test_select_grid():
    conds = [0, 1, -5, I64_MIN, 2**40]
    rows = [(c, vc, vb, ve) for c in conds for vc in (True, False)
            for vb in (True, False) for ve in (True, False)]
    cols = [[c if vc else GARBAGE for c, vc, _, _ in rows],
            [111 if vb else GARBAGE for _, _, vb, _ in rows],
            [I64_MAX if ve else GARBAGE for _, _, _, ve in rows]]
    valid = [np.array([r[i] for r in rows]) for i in (1, 2, 3)]
    want = check((3, [(MOP_SELECT, 0, 1, 3, 2)], [3], -1), cols, valid)
    assert set(want[0][0].tolist()) == {0, 111, I64_MAX}
    # dst may be the else-register itself
    check((3, [(MOP_SELECT, 0, 1, 2, 2)], [2], -1), cols, valid)


@pytest.mark.gpu
def test_const_is_valid_and_input_garbage_never_shows():
    """Outputs that are inputs: 0 under their NULLs, whatever came in."""
    cols = [[5, GARBAGE, I64_MAX, 7], [GARBAGE, GARBAGE, 1, 2]]
    valid = [np.array([True, False, False, True]),
             np.array([False, False, True, True])]
    want = check((2, [(MOP_CONST, 0, 0, 2, -3)], [0, 1, 2], -1), cols, valid)
    assert want[0][0].tolist() == [5, 0, 0, 7]
    assert want[1][2].all()


# ----------------------------------------------------------- GPU: error cases

@pytest.mark.gpu
def test_errors_only_where_the_result_is_valid():
    from arroyo_amd import gpu
    op = gpu.make_map_op(make_cfg(binary(MOP_DIV)))
    a, b = i64_cols([[1, 2, 3], [1, 0, 1]])
    yes, no = np.ones(3, dtype=bool), np.array([True, False, True])
    with pytest.raises(RuntimeError, match="division by zero"):
        op.process_batch_nullable([a, b], [yes, yes])
    # the same rows, the dividend of the x / 0 row NULL, then the divisor
    for valid in ([no, None], [None, no], [no, no]):
        cols, masks = op.process_batch_nullable([a, b], valid)
        assert cols[0].tolist() == [1, 0, 3]
        assert masks[0].tolist() == [True, False, True]
    with pytest.raises(RuntimeError, match="overflow"):
        op.process_batch_nullable(i64_cols([[I64_MIN], [-1]]), None)
    cols, masks = op.process_batch_nullable(
        i64_cols([[I64_MIN, 9], [-1, 3]]), [np.array([False, True]), None])
    assert cols[0].tolist() == [0, 3] and masks[0].tolist() == [False, True]
    op.close()
    op = gpu.make_map_op(make_cfg((1, [(MOP_F2I, 0, 0, 1)], [1], -1)))
    x = i64_cols([[f2b(1.5), f2b(math.inf)]])
    with pytest.raises(RuntimeError, match="cast"):
        op.process_batch_nullable(x, None)
    cols, masks = op.process_batch_nullable(x, [np.array([True, False])])
    assert cols[0].tolist() == [1, 0] and masks[0].tolist() == [True, False]
    op.close()


@pytest.mark.gpu
def test_guarded_division_idiom():
    """SELECT(b != 0, a / NULLIF(b, 0), -1): the machine is eager, so the
    division sees a NULL divisor, not a zero."""
    prog = [(MOP_CONST, 0, 0, 2, 0), (MOP_NE, 1, 2, 3),
            (MOP_NULLIF, 1, 2, 4), (MOP_DIV, 0, 4, 5),
            (MOP_CONST, 0, 0, 6, -1), (MOP_SELECT, 3, 5, 7, 6)]
    cols = [[7, 7, 7, -9, I64_MIN], [2, 0, 0, 0, -1]]
    valid = [None, np.array([True, True, False, True, False])]
    want = check((2, prog, [7], -1), cols, valid)
    assert want[0][0].tolist() == [3, -1, -1, -1, -1] and want[1][0].all()


# ------------------------------------------------------ random typed programs

N_PROGRAMS, N_ROWS, SEED = 40, 1061, 0
NONZERO_DIVISORS = [1, 2, 3, 7, 97, 1000, -2, -3, -97]


def gen_program(seed, length):
    """A typed program of exactly `length` instructions over old and new
    opcodes that passes validation and raises no row error on any input:
    divisors are non-zero constants, constants made NULL-able, or
    NULLIF(2 * (x % 7), 0); F2I reads only small floats.  Returns the
    program's config without a filter, its f64 flags and the registers that
    hold flags (filter candidates)."""
    rng = np.random.default_rng(seed)
    n_in = int(rng.integers(1, 5))
    typ = {r: "i" for r in range(n_in)}
    small, flags = set(), set()
    prog = []

    def pick(t, among=None):
        regs = [r for r in typ if typ[r] == t and
                (among is None or r in among)]
        return int(rng.choice(regs)) if regs else None

    def emit(op, a, b, t, imm=0, is_small=False, is_flag=False, dst=None):
        if dst is None:
            u = rng.random()
            if u < 0.1:
                dst = a
            elif u < 0.2:
                dst = int(rng.integers(0, n_in))     # overwrite an input
            elif u < 0.3:
                dst = MAX_REGS - 1
            else:
                dst = int(rng.integers(0, MAX_REGS))
        prog.append((op, a, b, dst, imm))
        typ[dst] = t
        (small.add if is_small else small.discard)(dst)
        (flags.add if is_flag else flags.discard)(dst)
        return dst

    def const_i(v, **kw):
        v = int(v)
        return emit(MOP_CONST, int(rng.integers(0, MAX_REGS)),
                    int(rng.integers(0, MAX_REGS)), "i", imm=v,
                    is_small=abs(v) <= 1000, **kw)

    def temp(*busy):
        free = [r for r in range(MAX_REGS) if r not in typ] or \
            [r for r in range(MAX_REGS) if r not in busy]
        return int(rng.choice(free))

    kinds = ["const_i", "const_f", "arith", "divmod", "cmp", "logic", "not",
             "i2f", "f2i", "farith", "is_null", "coalesce", "nullif",
             "select"]
    p = np.array([.06, .04, .12, .12, .08, .08, .03, .07, .05, .09, .07, .07,
                  .05, .07])
    while len(prog) < length:
        room = length - len(prog)
        kind = rng.choice(kinds, p=p / p.sum())
        a_i, b_i = pick("i"), pick("i")
        if kind == "const_i" or a_i is None:
            const_i(rng.choice([0, 1, -1, 3, 1000, 2**31, I64_MAX, I64_MIN,
                                int(rng.integers(-10**6, 10**6))]))
        elif kind == "const_f":
            emit(MOP_CONST, 0, 0, "f", imm=float(rng.choice(FLOAT_CONSTS)),
                 is_small=True)
        elif kind == "arith":
            emit(int(rng.choice([MOP_ADD, MOP_SUB, MOP_MUL])), a_i, b_i, "i")
        elif kind == "divmod":
            op = int(rng.choice([MOP_DIV, MOP_MOD]))
            u, t = rng.random(), temp(a_i, b_i)
            if room < 2:
                emit(MOP_SUB, a_i, b_i, "i")
            elif u < 0.4 or room < 3:
                d = const_i(rng.choice(NONZERO_DIVISORS), dst=t)
                emit(op, a_i, d, "i", is_small=op == MOP_MOD)
            elif u < 0.7 or room < 6:
                # a constant divisor that is NULL where it equals b
                d = const_i(rng.choice(NONZERO_DIVISORS), dst=t)
                emit(MOP_NULLIF, d, b_i, "i", dst=t, is_small=True)
                emit(op, a_i, t, "i", is_small=op == MOP_MOD)
            else:
                # NULLIF(2 * (b % 7), 0): even, so neither 0 nor -1
                seven = const_i(7, dst=t)
                emit(MOP_MOD, b_i, seven, "i", dst=t, is_small=True)
                emit(MOP_ADD, t, t, "i", dst=t, is_small=True)
                t2 = temp(a_i, b_i, t)
                zero = const_i(0, dst=t2)
                emit(MOP_NULLIF, t, zero, "i", dst=t, is_small=True)
                emit(op, a_i, t, "i", is_small=op == MOP_MOD)
        elif kind == "cmp":
            emit(int(rng.integers(MOP_EQ, MOP_GE + 1)), a_i, b_i, "i",
                 is_small=True, is_flag=True)
        elif kind == "logic":
            fa, fb = pick("i", flags), pick("i", flags)
            a, b = (fa, fb) if fa is not None and rng.random() < 0.8 \
                else (a_i, b_i)
            emit(int(rng.choice([MOP_AND, MOP_OR])), a, b, "i",
                 is_small=True, is_flag=True)
        elif kind == "not":
            emit(MOP_NOT, a_i, int(rng.integers(0, MAX_REGS)), "i",
                 is_small=True, is_flag=True)
        elif kind == "is_null":
            src = int(rng.choice(sorted(typ)))
            emit(int(rng.choice([MOP_IS_NULL, MOP_IS_NOT_NULL])), src,
                 int(rng.integers(0, MAX_REGS)), "i", is_small=True,
                 is_flag=True)
        elif kind == "nullif":
            # raw i64 compare: integer registers only (a NaN's payload is
            # not pinned)
            emit(MOP_NULLIF, a_i, b_i, "i", is_small=a_i in small,
                 is_flag=a_i in flags)
        elif kind in ("coalesce", "select"):
            t = "f" if rng.random() < 0.3 and pick("f") is not None else "i"
            x, y = pick(t), pick(t)
            both_small = x in small and y in small
            if kind == "coalesce":
                emit(MOP_COALESCE, x, y, t, is_small=both_small,
                     is_flag=x in flags and y in flags)
            else:
                cond = pick("i", flags) if rng.random() < 0.8 else None
                cond = a_i if cond is None else cond
                emit(MOP_SELECT, cond, x, t, imm=y, is_small=both_small,
                     is_flag=x in flags and y in flags)
        elif kind == "i2f":
            src = pick("i", small)
            src = a_i if src is None else src
            emit(MOP_I2F, src, int(rng.integers(0, MAX_REGS)), "f",
                 is_small=src in small)
        else:
            a_f, b_f = pick("f"), pick("f")
            if a_f is None:
                continue
            if kind == "f2i":
                src = pick("f", small)
                if src is None:
                    continue
                emit(MOP_F2I, src, int(rng.integers(0, MAX_REGS)), "i",
                     is_small=True)
            else:
                emit(int(rng.integers(MOP_FADD, MOP_FDIV + 1)), a_f, b_f, "f")

    regs = sorted(typ)
    n_out = int(rng.integers(1, 7))
    out_reg = [int(r) for r in rng.choice(regs, size=n_out)]
    out_is_f64 = [int(typ[r] == "f") for r in out_reg]
    return (n_in, prog, out_reg, -1), out_is_f64, sorted(flags) or regs


@functools.lru_cache(maxsize=None)
def random_case(i):
    length = MAX_PROG if i % 10 == 0 else 8 + (i * 23) % 57
    cfg, out_is_f64, flag_regs = gen_program(SEED + i, length)
    rng = np.random.default_rng(5000 + i)
    cols = gen_inputs(SEED + i, cfg[0])
    valid = [rng.random(N_ROWS) >= 0.3 for _ in cols]
    cols = [np.where(v, c, GARBAGE) for c, v in zip(cols, valid)]
    filtered = cfg[:3] + (int(rng.choice(flag_regs)),)
    return (cfg, filtered), out_is_f64, cols, valid, \
        (ref_eval(cfg, cols, valid), ref_eval(filtered, cols, valid))


def test_random_programs_cover_the_machine():
    """Conditions on the generated set, judged on the reference alone."""
    cases = [random_case(i) for i in range(N_PROGRAMS)]
    progs = [c[0][0][1] for c in cases]
    assert all(8 <= len(p) <= MAX_PROG for p in progs)
    assert any(len(p) == MAX_PROG for p in progs)
    assert {ins[0] for p in progs for ins in p} == set(range(MOP_SELECT + 1))
    assert any(ins[3] == MAX_REGS - 1 for p in progs for ins in p)
    # no case raises; about 30% NULLs in, NULLs and values out
    for c in cases:
        assert not isinstance(c[4][0], str), c[4][0]
        assert not isinstance(c[4][1], str), c[4][1]
        for v in c[3]:
            assert 0.2 < 1 - v.mean() < 0.4
    masks = [m for c in cases for m in c[4][0][1]]
    assert sum(0 < m.sum() < len(m) for m in masks) > len(masks) // 3
    assert any(m.all() for m in masks)
    # the filters are not trivial: some drop rows, and rows survive
    kept = [len(c[4][1][0][0]) for c in cases]
    assert sum(0 < k < N_ROWS for k in kept) >= N_PROGRAMS // 3


@pytest.mark.gpu
@pytest.mark.parametrize("filtered", [0, 1], ids=["nofilter", "filter"])
@pytest.mark.parametrize("i", range(N_PROGRAMS))
def test_random_program(i, filtered):
    cfgs, out_is_f64, cols, valid, wants = random_case(i)
    check(cfgs[filtered], cols, valid, out_is_f64, want=wants[filtered])


# ---------------------------------------------------- all-valid equivalence

@pytest.mark.gpu
@pytest.mark.parametrize("filter_reg", [-1, 6], ids=["nofilter", "filter"])
def test_all_valid_equals_null_semantics_off(filter_reg):
    """No new opcode, every input valid: the values of null_semantics = 0,
    and no bitmaps at all."""
    from arroyo_amd import gpu
    prog = [(MOP_CONST, 0, 0, 2, 97), (MOP_MOD, 0, 2, 3), (MOP_MUL, 0, 1, 4),
            (MOP_I2F, 1, 0, 5), (MOP_LT, 3, 1, 6), (MOP_AND, 6, 0, 7)]
    cfg = (2, prog, [4, 5, 3, 7, 0], filter_reg)
    f = [0, 1, 0, 0, 0]
    rng = np.random.default_rng(5)
    cols = [np.concatenate([rng.integers(I64_MIN, I64_MAX, size=N_ROWS -
                                         len(EI), endpoint=True),
                            EI]).astype(np.int64),
            rng.integers(-50, 50, size=N_ROWS).astype(np.int64)]
    off = gpu.make_map_op(make_cfg(cfg, f, ns=0))
    want = off.process_batch(cols)
    off.close()
    on = gpu.make_map_op(make_cfg(cfg, f, ns=1))
    all_true = dirty_bitmap(np.ones(N_ROWS, dtype=bool))
    for fn, bitmaps in (("process_batch", None),
                        ("process_batch_nullable", None),
                        ("process_batch_nullable", [None, all_true]),
                        ("process_batch_nullable", [all_true, all_true])):
        got, masks, has_table = raw_batch(on, fn, cols, bitmaps)
        assert not has_table and masks == [None] * 5
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert g.dtype == w.dtype
            assert np.array_equal(g.view(np.int64), w.view(np.int64))
    on.close()
    assert filter_reg < 0 or 0 < len(want[0]) < N_ROWS


# ------------------------------------------------- filter and launch shapes

# a row's flag is the predicate; `null_pred` keeps everything but NULLs the
# predicate of the dropped rows instead of zeroing it
PATTERNS = {
    "none": lambda ts: np.zeros(len(ts), dtype=bool),
    "all": lambda ts: np.ones(len(ts), dtype=bool),
    "first": lambda ts: ts == 0,
    "last": lambda ts: ts == len(ts) - 1,
    "alternating": lambda ts: ts % 2 == 1,
    "null_pred": lambda ts: ts % 5 != 2,
}

# the wave seam (64), the block seam (256) and the grid-stride seam: 2048
# blocks of 256 threads cover 524,288 rows in one pass
LAUNCH_SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 524_288, 524_289]


def shape_inputs(n):
    """x is NULL on every third row, and the NULLs of the outputs below sit
    on both sides of every seam."""
    ts = np.arange(n, dtype=np.int64)
    x = ts * 2654435761 - 17
    x_ok = ts % 3 != 0
    return ts, np.where(x_ok, x, GARBAGE), x_ok


# out: ts, x (nullable), NULLIF(ts % 7, 3) (makes its own NULLs),
# COALESCE(x, -1) (never NULL)
SHAPE_PROG = [(MOP_CONST, 0, 0, 3, 7), (MOP_MOD, 0, 3, 4),
              (MOP_CONST, 0, 0, 5, 3), (MOP_NULLIF, 4, 5, 6),
              (MOP_CONST, 0, 0, 7, -1), (MOP_COALESCE, 1, 7, 8)]
SHAPE_OUT = [0, 1, 6, 8]


def shape_want(ts, x, x_ok, keep):
    m7 = ts % 7
    cols = [ts, np.where(x_ok, x, 0), np.where(m7 != 3, m7, 0),
            np.where(x_ok, x, -1)]
    masks = [np.ones(len(ts), dtype=bool), x_ok, m7 != 3,
             np.ones(len(ts), dtype=bool)]
    return [c[keep] for c in cols], [m[keep] for m in masks]


def assert_shape(got, masks, has_table, want):
    wc, wm = want
    for i, (g, m, w, k) in enumerate(zip(got, masks, wc, wm)):
        assert np.array_equal(g, w), (i, np.flatnonzero(g != w)[:5])
        if k.all():
            assert m is None, (i, "bitmap on an all-valid column")
        else:
            assert m is not None and np.array_equal(m, k), i
    assert has_table == any(not k.all() for k in wm)


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n", LAUNCH_SIZES)
def test_filter_patterns(n, pattern):
    from arroyo_amd import gpu
    ts, x, x_ok = shape_inputs(n)
    keep = PATTERNS[pattern](ts)
    # -5 and I64_MIN + ts are as true as 1
    flag = np.where(keep, np.where(ts % 3 == 0, -5, I64_MIN + ts), 0)
    flag_ok = np.ones(n, dtype=bool)
    if pattern == "null_pred":
        flag, flag_ok = np.full(n, 1, dtype=np.int64), keep
    # every input bitmap with its padding bits set; _timestamp has one too
    bitmaps = [dirty_bitmap(np.ones(n, dtype=bool)), dirty_bitmap(x_ok),
               dirty_bitmap(flag_ok)]
    op = gpu.make_map_op(make_cfg((3, SHAPE_PROG, SHAPE_OUT, 2)))
    got, masks, has_table = raw_batch(op, "process_batch_nullable",
                                      [ts, x, flag], bitmaps)
    op.close()
    assert_shape(got, masks, has_table, shape_want(ts, x, x_ok, keep))


@pytest.mark.gpu
@pytest.mark.parametrize("n", LAUNCH_SIZES)
def test_no_filter_launch_sizes(n):
    from arroyo_amd import gpu
    ts, x, x_ok = shape_inputs(n)
    op = gpu.make_map_op(make_cfg((2, SHAPE_PROG, SHAPE_OUT, -1)))
    got, masks, has_table = raw_batch(
        op, "process_batch_nullable", [ts, x], [None, dirty_bitmap(x_ok)])
    op.close()
    assert_shape(got, masks, has_table,
                 shape_want(ts, x, x_ok, np.ones(n, dtype=bool)))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [CHUNK, CHUNK + 1, 2 * CHUNK + 3])
def test_host_chunk_seams(n):
    """The filter keeps ts % 3 != 1, so a chunk's kept count is no multiple
    of 8 and the next chunk's bitmap is appended at a bit offset; nullable
    outputs sit on both sides of each seam."""
    from arroyo_amd import gpu
    ts = np.arange(n, dtype=np.int64)
    x = ts * 2654435761 - 17
    x_ok = ts % 5 != 3          # row 2 * CHUNK + 1, kept, is a NULL
    x = np.where(x_ok, x, GARBAGE)
    prog = SHAPE_PROG + [(MOP_CONST, 0, 0, 9, 3), (MOP_MOD, 0, 9, 10),
                         (MOP_CONST, 0, 0, 11, 1), (MOP_NE, 10, 11, 12)]
    op = gpu.make_map_op(make_cfg((2, prog, SHAPE_OUT, 12)))
    got, masks, has_table = raw_batch(
        op, "process_batch_nullable", [ts, x], [None, dirty_bitmap(x_ok)])
    op.close()
    keep = ts % 3 != 1
    assert int(keep[:CHUNK].sum()) % 8 != 0
    want = shape_want(ts, x, x_ok, keep)
    for seam in range(CHUNK, n, CHUNK):
        at = int(keep[:seam].sum())             # first kept row past the seam
        n_kept = len(want[0][0])
        for k in want[1][1:3]:
            assert not k[at - 16:at].all()
        # past the seam: wherever rows were kept there (CHUNK + 1 keeps
        # none, 2 * CHUNK + 3 keeps two past its second seam)
        assert n_kept == at or not want[1][1][at:at + 16].all()
        assert n_kept - at < 16 or not want[1][2][at:at + 16].all()
    assert_shape(got, masks, has_table, want)


# -------------------------------------------- which call on which handle

@pytest.mark.gpu
def test_plain_call_on_a_null_handle_returns_bitmaps():
    """Every input valid, yet NULLIF makes NULLs: the plain call reports
    them."""
    from arroyo_amd import gpu
    cfg = (2, [(MOP_NULLIF, 0, 1, 2)], [2, 0], -1)
    op = gpu.make_map_op(make_cfg(cfg))
    cols = i64_cols([[1, 2, 3, 4], [1, 0, 3, 0]])
    got, masks, has_table = raw_batch(op, "process_batch", cols)
    assert has_table and masks[1] is None
    assert masks[0].tolist() == [False, True, False, True]
    assert got[0].tolist() == [0, 2, 0, 4] and got[1].tolist() == [1, 2, 3, 4]
    vals, ms = op.process_batch_with_validity(cols)
    assert ms[0].tolist() == [False, True, False, True] and ms[1].all()
    # the plain wrapper drops the masks, not the call
    assert op.process_batch(cols)[0].tolist() == [0, 2, 0, 4]
    op.close()


@pytest.mark.gpu
def test_nullable_call_on_a_plain_handle_is_an_error():
    from arroyo_amd import gpu
    op = gpu.make_map_op(make_cfg((1, [], [0], -1), ns=0))
    cols = i64_cols([[1, 2, 3]])
    with pytest.raises(RuntimeError, match="null_semantics = 0"):
        op.process_batch_nullable(cols, None)
    with pytest.raises(RuntimeError, match="null_semantics = 0"):
        op.process_batch_nullable(cols, [np.array([True, False, True])])
    with pytest.raises(RuntimeError, match="null_semantics = 0"):
        op.process_batch_nullable_device([0], None, 0)
    assert op.process_batch(cols)[0].tolist() == [1, 2, 3]
    op.close()


# ------------------------------------------------------------- device surface

class HipBytes(Hip):
    """Byte buffers next to the int64 ones of the opcode suite's helper."""

    def upload_bitmap(self, mask):
        """A bool mask as a device Arrow bitmap: 8-byte aligned (hipMalloc),
        padded to a multiple of 8 bytes, every padding bit set."""
        bm = dirty_bitmap(mask)
        padded = np.full((len(bm) + 7) // 8 * 8, 0xFF, dtype=np.uint8)
        padded[:len(bm)] = bm
        return self.upload(padded.view(np.int64))

    def download_bytes(self, ptr, nbytes):
        return self.download(ptr, nbytes // 8).view(np.uint8)


@pytest.fixture
def hip():
    h = HipBytes()
    yield h
    h.free()


def device_run(hip, op, cols, valid):
    """(values, masks, null counts) of the device surface; checks the
    returned bitmaps' alignment and padding on the way."""
    n = len(cols[0])
    dv = None if valid is None else \
        [None if v is None else hip.upload_bitmap(v) for v in valid]
    dptrs, dbms, nulls, n_keep = op.process_batch_nullable_device(
        [hip.upload(c) for c in cols], dv, n)
    vals = [hip.download(p, n_keep) for p in dptrs]
    masks = []
    for p in dbms:
        assert p and p % 8 == 0, "bitmap not 8-byte aligned"
        nbytes = (n_keep + 63) // 64 * 8
        raw = hip.download_bytes(p, nbytes)
        bits = np.unpackbits(raw, bitorder="little").astype(bool)
        assert not bits[n_keep:].any(), "padding bits up to 8 bytes not clear"
        masks.append(bits[:n_keep])
    return vals, masks, nulls


DEVICE_PROG = [(MOP_CONST, 0, 0, 2, 97), (MOP_MOD, 0, 2, 3),
               (MOP_MUL, 0, 1, 4), (MOP_I2F, 1, 0, 5), (MOP_LT, 3, 1, 6),
               (MOP_CONST, 0, 0, 7, 11), (MOP_NULLIF, 3, 7, 8),
               (MOP_COALESCE, 1, 3, 9), (MOP_IS_NULL, 4, 0, 10),
               (MOP_SELECT, 6, 0, 11, 8), (MOP_OR, 6, 10, 12)]
DEVICE_OUT = [4, 5, 8, 9, 10, 11]
DEVICE_F64 = [0, 1, 0, 0, 0, 0]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1061, 64, 0])
@pytest.mark.parametrize("filter_reg", [-1, 12], ids=["nofilter", "filter"])
def test_device_surface_matches_reference_and_host(hip, filter_reg, n):
    from arroyo_amd import gpu
    rng = np.random.default_rng(5)
    big = np.concatenate([rng.integers(I64_MIN, I64_MAX, size=max(n, len(EI)),
                                       endpoint=True), EI])[-n:] if n else []
    cols = [np.array(big, dtype=np.int64),
            rng.integers(-50, 50, size=n).astype(np.int64)]
    valid = [rng.random(n) >= 0.3, rng.random(n) >= 0.3]
    cols = [np.where(v, c, GARBAGE) for c, v in zip(cols, valid)]
    cfg = (2, DEVICE_PROG, DEVICE_OUT, filter_reg)
    want = ref_eval(cfg, cols, valid)
    if n == 1061:
        assert filter_reg < 0 or 0 < len(want[0][0]) < n
        assert sum(0 < m.sum() < len(m) for m in want[1]) >= 3
    op = gpu.make_map_op(make_cfg(cfg, DEVICE_F64))
    vals, masks, nulls = device_run(hip, op, cols, valid)
    host = op.process_batch_nullable(cols, valid)
    # one column without a bitmap, and none at all: all valid
    v1, m1, _ = device_run(hip, op, cols, [None, valid[1]])
    v2, m2, n2 = device_run(hip, op, cols, None)
    op.close()
    got = ([v.view(np.float64) if f else v
            for v, f in zip(vals, DEVICE_F64)], masks)
    assert_result(got, want, DEVICE_F64)
    assert_result(host, want, DEVICE_F64)
    assert nulls == [int((~m).sum()) for m in want[1]]
    w1 = ref_eval(cfg, [np.where(valid[0], cols[0], GARBAGE), cols[1]],
                  [None, valid[1]])
    for v, m, w, k in zip(v1, m1, *w1):
        assert np.array_equal(m, k)
    # with every input valid the garbage is data: compare on its own terms
    w2 = ref_eval(cfg, cols, None)
    assert n2 == [int((~m).sum()) for m in w2[1]]
    assert all(np.array_equal(m, k) for m, k in zip(m2, w2[1]))


@pytest.mark.gpu
def test_device_surface_wrong_shape_calls_and_recovery(hip):
    from arroyo_amd import gpu
    cfg = (2, [(MOP_DIV, 0, 1, 2)], [2], -1)
    op = gpu.make_map_op(make_cfg(cfg))
    cols = i64_cols([[7, -7, 9, I64_MIN], [2, 2, -3, 1]])
    valid = [np.array([True, False, True, True]), None]
    want = ref_eval(cfg, cols, valid)

    def good():
        vals, masks, nulls = device_run(hip, op, cols, valid)
        assert_result((vals, masks), want)
        assert vals[0].tolist() == [3, 0, -3, I64_MIN] and nulls == [1]

    good()
    d = hip.upload([1, 2, 3])
    # the plain device call cannot return bitmaps
    with pytest.raises(RuntimeError, match="nullable_device"):
        op.process_batch_device([d, d], 3)
    good()
    with pytest.raises(RuntimeError, match="exceeds capacity"):
        op.process_batch_nullable_device([d, d], None, CHUNK + 1)
    good()
    with pytest.raises(RuntimeError, match="expected 2 cols"):
        op.process_batch_nullable_device([d], None, 3)
    with pytest.raises(RuntimeError, match="8-byte aligned"):
        op.process_batch_nullable_device([d, d], [d + 4, None], 3)
    good()
    # a row error fails the call; the next batch is judged afresh
    with pytest.raises(RuntimeError, match="division by zero"):
        device_run(hip, op, i64_cols([[1, 2, 3], [1, 0, 1]]), None)
    good()
    op.close()
