"""Every map opcode against an independent reference, at the i64 / f64 edges.

`ref_eval` below is written from the semantics table in
include/arroyo_amd_types.h (restated from arrow-arith / DataFusion, see
COVERAGE.md row 3), on Python `int` (arbitrary precision, wrapped to 64 bits
explicitly) and Python `float`.  It shares no code with the oracle's or the
kernel's `switch`.  Every case runs against the CPU oracle and, marked `gpu`,
against the HIP operator; both are compared with `ref_eval` (or with numpy
for the launch-shape cases), never with each other."""
import ctypes
import functools
import math
import struct

import numpy as np
import pytest

import oracle
from arroyo_amd import cabi
from arroyo_amd.cabi import (MOP_ADD, MOP_AND, MOP_CONST, MOP_DIV, MOP_EQ,
                             MOP_F2I, MOP_FADD, MOP_FDIV, MOP_FMUL, MOP_FSUB,
                             MOP_GE, MOP_GT, MOP_I2F, MOP_LE, MOP_LT, MOP_MOD,
                             MOP_MUL, MOP_NE, MOP_NOT, MOP_OR, MOP_SUB)

I64_MIN, I64_MAX = -2**63, 2**63 - 1
MAX_PROG, MAX_REGS = 64, 32

BACKENDS = [pytest.param("oracle"),
            pytest.param("hip", marks=pytest.mark.gpu)]


@pytest.fixture(params=BACKENDS)
def mod(request):
    if request.param == "oracle":
        return oracle
    from arroyo_amd import gpu
    return gpu


# ------------------------------------------------------------ the reference

def f2b(f):
    return struct.unpack("<q", struct.pack("<d", f))[0]


def b2f(b):
    return struct.unpack("<d", struct.pack("<q", b))[0]


def wrap(x):
    x &= 2**64 - 1
    return x - 2**64 if x >= 2**63 else x


class RowError(Exception):
    pass


def _fdiv(x, y):
    if y != 0.0:
        return x / y
    if x != x or x == 0.0:
        return math.nan
    return math.copysign(math.inf, x) * math.copysign(1.0, y)


def _int_op(op, a, b):
    if op == MOP_ADD:
        return wrap(a + b)
    if op == MOP_SUB:
        return wrap(a - b)
    if op == MOP_MUL:
        return wrap(a * b)
    if op in (MOP_DIV, MOP_MOD):
        if b == 0:
            raise RowError("division by zero")
        q, r = divmod(abs(a), abs(b))           # magnitude, then the sign
        if op == MOP_MOD:
            return -r if a < 0 else r           # sign of the dividend
        q = -q if (a < 0) != (b < 0) else q     # truncation toward zero
        if not I64_MIN <= q <= I64_MAX:
            raise RowError("overflow")
        return q
    if op == MOP_AND:
        return int(a != 0 and b != 0)
    if op == MOP_OR:
        return int(a != 0 or b != 0)
    return int({MOP_EQ: a == b, MOP_NE: a != b, MOP_LT: a < b,
                MOP_LE: a <= b, MOP_GT: a > b, MOP_GE: a >= b}[op])


def _float_op(op, x, y):
    if op == MOP_FDIV:
        return _fdiv(x, y)
    return {MOP_FADD: x + y, MOP_FSUB: x - y, MOP_FMUL: x * y}[op]


def _eval_row(prog, regs):
    for ins in prog:
        op, a, b, dst = ins[:4]
        if op == MOP_CONST:
            imm = ins[4] if len(ins) > 4 else 0
            v = f2b(imm) if isinstance(imm, float) else imm
        elif op == MOP_NOT:
            v = int(regs[a] == 0)
        elif op == MOP_I2F:
            v = f2b(float(regs[a]))             # int -> float rounds RNE
        elif op == MOP_F2I:
            x = b2f(regs[a])
            if not math.isfinite(x) or not I64_MIN <= math.trunc(x) <= I64_MAX:
                raise RowError("cast")
            v = math.trunc(x)
        elif op >= MOP_FADD:
            v = f2b(_float_op(op, b2f(regs[a]), b2f(regs[b])))
        else:
            v = _int_op(op, regs[a], regs[b])
        regs[dst] = v


def ref_eval(cfg, cols):
    """cfg = (n_in_cols, prog, out_reg, filter_reg), prog as make_map_config
    takes it; cols = input columns of ints.  Returns the output columns as
    lists of signed 64-bit patterns, or the kind of error the batch raises.
    A register holds nothing before it is written (a KeyError here)."""
    n_in, prog, out_reg, filter_reg = cfg
    assert len(cols) == n_in
    outs, kinds = [[] for _ in out_reg], set()
    for row in zip(*[[int(v) for v in c] for c in cols]):
        regs = dict(enumerate(row))
        try:
            _eval_row(prog, regs)
        except RowError as e:
            kinds.add(e.args[0])
            continue
        if filter_reg >= 0 and regs[filter_reg] == 0:
            continue
        for o, r in zip(outs, out_reg):
            o.append(regs[r])
    # which error a batch of mixed errors reports is unspecified
    assert len(kinds) <= 1, f"test batch mixes error kinds: {kinds}"
    return kinds.pop() if kinds else outs


def test_ref_eval_literals():
    """The reference itself, against results worked out by hand."""
    def one(op, a, b=0):
        out = ref_eval((2, [(op, 0, 1, 2)], [2], -1), [[a], [b]])
        return out if isinstance(out, str) else out[0][0]
    assert one(MOP_ADD, I64_MAX, 1) == I64_MIN
    assert one(MOP_SUB, I64_MIN, 1) == I64_MAX
    assert one(MOP_MUL, I64_MIN, -1) == I64_MIN
    assert one(MOP_MUL, 2**32, 2**32) == 0
    assert one(MOP_MUL, 2**53 + 1, 2**53 + 1) == 2**54 + 1
    assert one(MOP_DIV, -7, 2) == -3 and one(MOP_DIV, 7, -2) == -3
    assert one(MOP_MOD, -7, 2) == -1 and one(MOP_MOD, 7, -2) == 1
    assert one(MOP_DIV, I64_MIN, -1) == "overflow"
    assert one(MOP_MOD, I64_MIN, -1) == 0
    assert one(MOP_DIV, 1, 0) == "division by zero"
    assert one(MOP_MOD, 1, 0) == "division by zero"
    assert one(MOP_LT, I64_MIN, I64_MAX) == 1 and one(MOP_GE, -1, 0) == 0
    assert one(MOP_AND, I64_MIN, -1) == 1 and one(MOP_OR, 0, 0) == 0
    assert one(MOP_NOT, I64_MIN) == 0 and one(MOP_NOT, 0) == 1
    assert one(MOP_I2F, 2**53 + 1) == f2b(2.0**53)          # tie -> even
    assert one(MOP_I2F, 2**53 + 3) == f2b(2.0**53 + 4)
    assert one(MOP_I2F, I64_MAX) == f2b(2.0**63)
    assert one(MOP_F2I, f2b(-0.5)) == 0 and one(MOP_F2I, f2b(-1.5)) == -1
    assert one(MOP_F2I, f2b(-2.0**63)) == I64_MIN
    assert one(MOP_F2I, f2b(2.0**63)) == "cast"
    assert one(MOP_F2I, f2b(math.nan)) == "cast"
    assert one(MOP_FDIV, f2b(1.0), f2b(-0.0)) == f2b(-math.inf)
    assert one(MOP_FMUL, f2b(5e-324), f2b(0.5)) == f2b(0.0)  # tie -> even
    assert one(MOP_FMUL, f2b(5e-324), f2b(1.5)) == f2b(1e-323)


# --------------------------------------------------------------- the harness

def make_cfg(cfg, out_is_f64=None):
    n_in, prog, out_reg, filter_reg = cfg
    return cabi.make_map_config(n_in_cols=n_in, prog=prog, out_reg=out_reg,
                                out_is_f64=out_is_f64, filter_reg=filter_reg)


def i64_cols(cols):
    return [np.array(c, dtype=np.int64) for c in cols]


def error_kind(exc):
    msg = str(exc)
    for kind in ("division by zero", "overflow", "cast"):
        if kind in msg:
            return kind
    raise exc


def run(mod, cfg, cols, out_is_f64=None):
    """The operator's output columns, or the kind of error it raised."""
    op = mod.make_map_op(make_cfg(cfg, out_is_f64))
    try:
        return op.process_batch(i64_cols(cols))
    except RuntimeError as e:
        return error_kind(e)
    finally:
        op.close()


def assert_cols(got, want, out_is_f64=None):
    """Bit-exact, except that where an f64 result is NaN both sides must be
    NaN (payload and sign not compared)."""
    assert not isinstance(got, str), f"raised {got!r}"
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        f = bool(out_is_f64 and out_is_f64[i])
        assert g.dtype == (np.float64 if f else np.int64)
        gb, wb = g.view(np.int64), np.array(w, dtype=np.int64)
        assert gb.shape == wb.shape
        if f:
            nan = np.isnan(wb.view(np.float64))
            assert np.array_equal(np.isnan(g), nan)
            gb, wb = gb[~nan], wb[~nan]
        bad = np.flatnonzero(gb != wb)
        assert bad.size == 0, (i, bad[:5], gb[bad[:5]], wb[bad[:5]])


def check(mod, cfg, cols, out_is_f64=None, want=None):
    want = ref_eval(cfg, cols) if want is None else want
    got = run(mod, cfg, cols, out_is_f64)
    if isinstance(want, str):
        assert isinstance(got, str), f"no error, want {want!r}"
        assert got == want
    else:
        assert_cols(got, want, out_is_f64)
    return want


# --------------------------------------------------------- integer edge grid

EI = [0, 1, -1, 2, -2, 3, -3, 97, -97, 2**31 - 1, 2**31, -2**31, 2**32,
      2**53, 2**53 + 1, -(2**53 + 1), I64_MAX, I64_MAX - 1, I64_MIN,
      I64_MIN + 1]
EI_PAIRS = [(a, b) for a in EI for b in EI]

BIN_INT_OPS = {"ADD": MOP_ADD, "SUB": MOP_SUB, "MUL": MOP_MUL, "EQ": MOP_EQ,
               "NE": MOP_NE, "LT": MOP_LT, "LE": MOP_LE, "GT": MOP_GT,
               "GE": MOP_GE, "AND": MOP_AND, "OR": MOP_OR}


def binary(op):
    return (2, [(op, 0, 1, 2)], [2], -1)


def unary(op):
    return (1, [(op, 0, 0, 1)], [1], -1)


def columns(pairs):
    return [[p[0] for p in pairs], [p[1] for p in pairs]]


@functools.lru_cache(maxsize=None)
def int_grid_want(op):
    return ref_eval(binary(op), columns(EI_PAIRS))


@pytest.mark.parametrize("name", BIN_INT_OPS)
def test_int_grid_binary(mod, name):
    op = BIN_INT_OPS[name]
    want = check(mod, binary(op), columns(EI_PAIRS), want=int_grid_want(op))
    if op >= MOP_EQ:
        assert set(want[0]) == {0, 1}           # exactly 0 or 1


def test_int_grid_not(mod):
    want = check(mod, unary(MOP_NOT), [EI])
    assert want[0] == [int(v == 0) for v in EI]


def test_int_grid_i2f(mod):
    check(mod, unary(MOP_I2F), [EI], out_is_f64=[1])


def divmod_ok_pairs(op):
    return [(a, b) for a, b in EI_PAIRS
            if b != 0 and not (op == MOP_DIV and (a, b) == (I64_MIN, -1))]


@pytest.mark.parametrize("op", [MOP_DIV, MOP_MOD], ids=["DIV", "MOD"])
def test_int_grid_divmod(mod, op):
    pairs = divmod_ok_pairs(op)
    want = check(mod, binary(op), columns(pairs))
    assert len(want[0]) == len(pairs)
    if op == MOP_MOD:
        assert want[0][pairs.index((I64_MIN, -1))] == 0
        assert all(w == 0 for w, p in zip(want[0], pairs) if p[1] == -1)


@pytest.mark.parametrize("op", [MOP_DIV, MOP_MOD], ids=["DIV", "MOD"])
def test_int_grid_div_by_zero(mod, op):
    pairs = divmod_ok_pairs(op)
    pairs.insert(len(pairs) // 2, (5, 0))
    assert check(mod, binary(op), columns(pairs)) == "division by zero"


def test_int_grid_div_overflow(mod):
    pairs = divmod_ok_pairs(MOP_DIV) + [(I64_MIN, -1)]
    assert check(mod, binary(MOP_DIV), columns(pairs)) == "overflow"


def test_compares_are_integer_compares(mod):
    """There are no float compares: f64 bit patterns compare as the signed
    integers they are.  -0.0 < 0.0, NaN == NaN, -1.0 < -2.0."""
    nan = f2b(math.nan)
    pairs = [(f2b(-0.0), f2b(0.0)), (nan, nan), (f2b(-1.0), f2b(-2.0)),
             (f2b(0.0), f2b(-0.0))]
    for op, expect in ((MOP_LT, [1, 0, 1, 0]), (MOP_EQ, [0, 1, 0, 0]),
                       (MOP_GE, [0, 1, 0, 1])):
        want = check(mod, binary(op), columns(pairs))
        assert want[0] == expect


# ----------------------------------------------------------- float edge grid

TWO63 = 2.0**63
EF = [0.0, -0.0, 0.5, -0.5, 1.0, -1.0, 1.5, -1.5, 2.5, 0.908, 1 / 3,
      5e-324, -5e-324, b2f(0x000FFFFFFFFFFFFF), 2.2250738585072014e-308,
      1.7976931348623157e308, -1.7976931348623157e308, math.inf, -math.inf,
      math.nan, 2.0**53, 2.0**53 + 2, float(np.nextafter(TWO63, 0.0)), TWO63,
      -TWO63, float(np.nextafter(-TWO63, -math.inf)), 1e19, -1e19]
EF_BITS = [f2b(x) for x in EF]
EF_PAIRS = [(a, b) for a in EF_BITS for b in EF_BITS]
EF_CASTABLE = [math.isfinite(x) and -TWO63 <= x < TWO63 for x in EF]

FLOAT_OPS = {"FADD": MOP_FADD, "FSUB": MOP_FSUB, "FMUL": MOP_FMUL,
             "FDIV": MOP_FDIV}


@functools.lru_cache(maxsize=None)
def float_grid_want(op):
    return ref_eval(binary(op), columns(EF_PAIRS))


@pytest.mark.parametrize("name", FLOAT_OPS)
def test_float_grid(mod, name):
    op = FLOAT_OPS[name]
    want = check(mod, binary(op), columns(EF_PAIRS), out_is_f64=[1],
                 want=float_grid_want(op))
    # the grid reaches subnormal and NaN results
    vals = [b2f(w) for w in want[0]]
    assert any(v != v for v in vals)
    assert any(0.0 < abs(v) < 2.2250738585072014e-308 for v in vals)


def test_float_grid_f2i_in_range(mod):
    bits = [b for b, ok in zip(EF_BITS, EF_CASTABLE) if ok]
    want = check(mod, unary(MOP_F2I), [bits])
    assert len(want[0]) == len(bits) == len(EF) - 9
    assert I64_MIN in want[0] and 2**63 - 1024 in want[0]


@pytest.mark.parametrize(
    "x", [x for x, ok in zip(EF, EF_CASTABLE) if not ok], ids=repr)
def test_float_grid_f2i_out_of_range(mod, x):
    assert check(mod, unary(MOP_F2I), [[f2b(1.0), f2b(x), f2b(2.0)]]) == "cast"


# ------------------------------------------------------ random typed programs

N_PROGRAMS, N_ROWS, SEED = 40, 1061, 0
SMALL_DIVISORS = [1, 2, 3, 7, 97, 1000, -2, -3, -97]
FLOAT_CONSTS = [0.908, 0.5, -1.5, 3.0, 1e-3, -7.25, 1 / 3, 1e6]


def gen_program(seed, length, with_filter):
    """A program of exactly `length` instructions that passes validation.
    Tracks each register's type, so i64 ops read i64 registers and f64 ops
    f64 registers, and which registers are known to be small, so that most
    F2I inputs are in range; most divisors are non-zero by construction."""
    rng = np.random.default_rng(seed)
    n_in = int(rng.integers(1, 5))
    typ = {r: "i" for r in range(n_in)}
    small, flags = set(), set()
    prog = []

    def pick(t, prefer=None):
        regs = [r for r in typ if typ[r] == t]
        pref = [r for r in regs if prefer and r in prefer]
        if pref and rng.random() < 0.9:
            regs = pref
        return int(rng.choice(regs)) if regs else None

    def emit(op, a, b, t, imm=0, is_small=False, is_flag=False, dst=None):
        if dst is None:
            u = rng.random()
            if u < 0.15:
                dst = a                          # dst == a
            elif u < 0.25:
                dst = int(rng.integers(0, n_in))  # overwrite an input
            elif u < 0.35:
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
        """a register for a temporary: an unused one while there is one"""
        free = [r for r in range(MAX_REGS) if r not in typ] or \
            [r for r in range(MAX_REGS) if r not in busy]
        return int(rng.choice(free))

    while len(prog) < length:
        room = length - len(prog)
        kind = rng.choice(["const_i", "const_f", "arith", "divmod", "cmp",
                           "logic", "not", "i2f", "f2i", "farith"],
                          p=[.08, .06, .16, .14, .12, .08, .05, .10, .07, .14])
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
            if room >= 2 and u < 0.6:
                d = const_i(rng.choice(SMALL_DIVISORS), dst=t)
                emit(op, a_i, d, "i", is_small=op == MOP_MOD)
            elif u < 0.98 and room < 4:
                emit(MOP_SUB, a_i, b_i, "i")
            elif u < 0.98:
                # b + (b == 0): never zero
                z = const_i(0, dst=t)
                emit(MOP_EQ, b_i, z, "i", dst=t)
                emit(MOP_ADD, b_i, t, "i", dst=t)
                emit(op, a_i, t, "i")
            else:
                emit(op, a_i, b_i, "i")          # may divide by zero
        elif kind == "cmp":
            emit(int(rng.integers(MOP_EQ, MOP_GE + 1)), a_i, b_i, "i",
                 is_small=True, is_flag=True)
        elif kind == "logic":
            emit(int(rng.choice([MOP_AND, MOP_OR])), a_i, b_i, "i",
                 is_small=True, is_flag=True)
        elif kind == "not":
            emit(MOP_NOT, a_i, int(rng.integers(0, MAX_REGS)), "i",
                 is_small=True, is_flag=True)
        elif kind == "i2f":
            src = pick("i", prefer=small)
            emit(MOP_I2F, src, int(rng.integers(0, MAX_REGS)), "f",
                 is_small=src in small)
        else:
            a_f, b_f = pick("f", prefer=small), pick("f")
            if a_f is None:
                continue
            if kind == "f2i":
                emit(MOP_F2I, a_f, int(rng.integers(0, MAX_REGS)), "i",
                     is_small=a_f in small)
            else:
                emit(int(rng.integers(MOP_FADD, MOP_FDIV + 1)), a_f, b_f, "f")

    regs = sorted(typ)
    n_out = int(rng.integers(1, 7))
    out_reg = [int(r) for r in rng.choice(regs, size=n_out)]
    out_is_f64 = [int(typ[r] == "f") for r in out_reg]
    filter_reg = -1
    if with_filter:
        filter_reg = int(rng.choice(sorted(flags) if flags else regs))
    return (n_in, prog, out_reg, filter_reg), out_is_f64


def gen_inputs(seed, n_in):
    """one third full range, one third |x| < 1000, one third from EI"""
    rng = np.random.default_rng(1000 + seed)
    third = N_ROWS // 3
    cols = []
    for _ in range(n_in):
        cols.append(np.concatenate([
            rng.integers(I64_MIN, I64_MAX, size=third, endpoint=True),
            rng.integers(-999, 1000, size=third),
            rng.choice(np.array(EI, dtype=np.int64), size=N_ROWS - 2 * third),
        ]).astype(np.int64))
    order = rng.permutation(N_ROWS)
    return [c[order] for c in cols]


@functools.lru_cache(maxsize=None)
def random_case(i):
    length = MAX_PROG if i % 10 == 0 else 8 + (i * 23) % 57
    cfg, out_is_f64 = gen_program(SEED + i, length, i % 2 == 1)
    cols = gen_inputs(SEED + i, cfg[0])
    return cfg, out_is_f64, cols, ref_eval(cfg, [c.tolist() for c in cols])


def test_random_programs_cover_the_machine():
    """Conditions on the generated set, judged on the reference alone."""
    cases = [random_case(i) for i in range(N_PROGRAMS)]
    progs = [c[0][1] for c in cases]
    assert all(8 <= len(p) <= MAX_PROG for p in progs)
    assert any(len(p) == MAX_PROG for p in progs)
    assert {ins[0] for p in progs for ins in p} == set(range(MOP_FDIV + 1))
    assert any(ins[3] == MAX_REGS - 1 for p in progs for ins in p)
    assert any(ins[1] == MAX_REGS - 1
               for p in progs for ins in p if ins[0] != MOP_CONST)
    assert {len(c[0][2]) for c in cases} == set(range(1, 7))
    assert sum(c[0][3] >= 0 for c in cases) == N_PROGRAMS // 2
    raising = [i for i, c in enumerate(cases) if isinstance(c[3], str)]
    assert len(raising) <= 10, raising
    # the filters are not trivial: some drop rows, and rows survive
    kept = [len(c[3][0]) for c in cases
            if c[0][3] >= 0 and not isinstance(c[3], str)]
    assert any(0 < k < N_ROWS for k in kept)


@pytest.mark.parametrize("i", range(N_PROGRAMS))
def test_random_program(mod, i):
    cfg, out_is_f64, cols, want = random_case(i)
    check(mod, cfg, cols, out_is_f64, want=want)


# ------------------------------------------------------------------ structure

def test_empty_program_reorders_and_duplicates(mod):
    cols = [[1, 2, 3], [40, 50, 60]]
    want = check(mod, (2, [], [1, 1, 0], -1), cols)
    assert want == [cols[1], cols[1], cols[0]]


def test_dst_equal_a_and_overwritten_input(mod):
    prog = [(MOP_ADD, 0, 1, 0),          # r0 += r1: dst == a, input overwritten
            (MOP_MUL, 0, 0, 0),          # r0 *= r0
            (MOP_SUB, 1, 0, 1)]          # r1 = r1 - r0
    want = check(mod, (2, prog, [0, 1], -1), [[1, -2, I64_MAX], [2, 5, 1]])
    assert want == [[9, 9, 0], [-7, -4, 1]]


def test_six_outputs(mod):
    prog = [(MOP_ADD, 0, 1, 2), (MOP_SUB, 0, 1, 3), (MOP_I2F, 0, 0, 4),
            (MOP_LT, 0, 1, 5)]
    cols = [EI, EI[::-1]]
    for filter_reg in (-1, 5):
        check(mod, (2, prog, [5, 4, 3, 2, 1, 0], filter_reg), cols,
              out_is_f64=[0, 1, 0, 0, 0, 0])


def test_f64_flag_selects_the_array_dtype(mod):
    prog = [(MOP_I2F, 0, 0, 1), (MOP_CONST, 0, 0, 2, 0.908),
            (MOP_FMUL, 1, 2, 3)]
    op = mod.make_map_op(make_cfg((1, prog, [3, 3, 0], -1), [1, 0, 0]))
    out = op.process_batch(i64_cols([[1000, -3]]))
    op.close()
    assert [o.dtype for o in out] == [np.float64, np.int64, np.int64]
    assert out[0].tolist() == [1000 * 0.908, -3 * 0.908]
    assert out[1].tolist() == [f2b(1000 * 0.908), f2b(-3 * 0.908)]


def test_filter_is_an_integer_test_of_the_register(mod):
    """-0.0 is a non-zero bit pattern, so a filter on it keeps the row."""
    cols = [[f2b(-0.0), f2b(0.0), f2b(math.nan), 0, I64_MIN, 1]]
    want = check(mod, (1, [], [0], 0), cols)
    assert want == [[f2b(-0.0), f2b(math.nan), I64_MIN, 1]]


def test_registers_do_not_carry_over_between_rows(mod):
    """A register overwritten in one row starts from the input again in the
    next: running sum needs state the machine does not have."""
    prog = [(MOP_CONST, 0, 0, 5, 0), (MOP_ADD, 5, 0, 5)]
    want = check(mod, (1, prog, [5], -1), [[1, 2, 3]])
    assert want == [[1, 2, 3]]


# ------------------------------------------------- filter and launch shapes

PATTERNS = {
    "none": lambda ts: np.zeros(len(ts), dtype=bool),
    "all": lambda ts: np.ones(len(ts), dtype=bool),
    "first": lambda ts: ts == 0,
    "last": lambda ts: ts == len(ts) - 1,
    "alternating": lambda ts: ts % 2 == 1,
}

# 2048 blocks of 256 threads: 524,288 is the last size one pass of the
# grid-stride loop covers
LAUNCH_SIZES = [1, 255, 256, 257, 524_288, 524_289]


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n", LAUNCH_SIZES)
def test_filter_patterns(mod, n, pattern):
    ts = np.arange(n, dtype=np.int64)
    keep = PATTERNS[pattern](ts)
    # -5 and I64_MIN are as true as 1
    flag = np.where(keep, np.where(ts % 3 == 0, -5, I64_MIN + ts), 0)
    prog = [(MOP_CONST, 0, 0, 2, 7), (MOP_MUL, 0, 2, 3)]
    op = mod.make_map_op(make_cfg((2, prog, [0, 3], 1)))
    out = op.process_batch([ts, flag.astype(np.int64)])
    op.close()
    assert len(out) == 2
    assert np.array_equal(out[0], ts[keep])
    assert np.array_equal(out[1], ts[keep] * 7)


@pytest.mark.parametrize("n", LAUNCH_SIZES)
def test_no_filter_launch_sizes(mod, n):
    ts = np.arange(n, dtype=np.int64)
    op = mod.make_map_op(make_cfg((1, [(MOP_SUB, 0, 0, 1),
                                       (MOP_SUB, 1, 0, 1)], [1, 0], -1)))
    out = op.process_batch([ts])
    op.close()
    assert np.array_equal(out[0], -ts) and np.array_equal(out[1], ts)


CHUNK = 1 << 20     # rows the host surface stages per launch


@pytest.mark.parametrize("n", [CHUNK, CHUNK + 1, 2 * CHUNK + 3])
def test_host_chunk_seams(mod, n):
    """Kept rows straddle both seams of the host surface's chunking."""
    ts = np.arange(n, dtype=np.int64)
    x = ts * 2654435761 - 17
    prog = [(MOP_CONST, 0, 0, 2, 3), (MOP_MOD, 1, 2, 3),
            (MOP_CONST, 0, 0, 4, 1), (MOP_NE, 3, 4, 5), (MOP_ADD, 0, 1, 6)]
    op = mod.make_map_op(make_cfg((2, prog, [6, 1], 5)))
    out = op.process_batch([x, ts])
    op.close()
    keep = ts % 3 != 1
    assert keep[CHUNK - 1] or keep[CHUNK]
    assert np.array_equal(out[1], ts[keep])
    assert np.array_equal(out[0], (x + ts)[keep])


# ------------------------------------------------------------ error recovery

def test_error_word_is_cleared_when_reported(mod):
    """A failed batch returns nothing, and the next batch on the same handle
    is evaluated afresh."""
    op = mod.make_map_op(make_cfg(binary(MOP_DIV)))
    good = i64_cols([[7, -7, 9], [2, 2, -3]])
    with pytest.raises(RuntimeError, match="division by zero"):
        op.process_batch(i64_cols([[1, 2, 3], [1, 0, 1]]))
    assert op.process_batch(good)[0].tolist() == [3, -3, -3]
    with pytest.raises(RuntimeError, match="overflow"):
        op.process_batch(i64_cols([[I64_MIN], [-1]]))
    assert op.process_batch(good)[0].tolist() == [3, -3, -3]
    op.close()


# ------------------------------------------------------------- device surface

class Hip:
    """Device buffers through the HIP runtime the operator library itself
    loaded, by ctypes: uploads and read-backs that do not go through the map
    operator."""

    def __init__(self):
        from arroyo_amd import gpu
        gpu.lib()
        # a symbol lookup on the library's handle also searches what it
        # links, so this reaches exactly the runtime its buffers live in
        self.rt = ctypes.CDLL(gpu._SO)
        vp, sz = ctypes.c_void_p, ctypes.c_size_t
        self.rt.hipMalloc.argtypes = [ctypes.POINTER(vp), sz]
        self.rt.hipMemcpy.argtypes = [vp, vp, sz, ctypes.c_int]
        self.rt.hipFree.argtypes = [vp]
        self.bufs = []

    def upload(self, values):
        a = np.ascontiguousarray(values, dtype=np.int64)
        p = ctypes.c_void_p()
        assert self.rt.hipMalloc(ctypes.byref(p), max(a.nbytes, 8)) == 0
        self.bufs.append(p)
        if a.nbytes:
            assert self.rt.hipMemcpy(p, a.ctypes.data, a.nbytes, 1) == 0
        return p.value

    def download(self, ptr, n):
        a = np.empty(n, dtype=np.int64)
        if n:
            assert self.rt.hipMemcpy(a.ctypes.data, ptr, a.nbytes, 2) == 0
        return a

    def free(self):
        for p in self.bufs:
            self.rt.hipFree(p)
        self.bufs = []


@pytest.fixture
def hip():
    h = Hip()
    yield h
    h.free()


def device_run(hip, op, cols):
    n = len(cols[0])
    dptrs, n_keep = op.process_batch_device(
        [hip.upload(c) for c in cols], n)
    return [hip.download(p, n_keep) for p in dptrs]


DEVICE_PROG = [(MOP_CONST, 0, 0, 2, 97), (MOP_MOD, 0, 2, 3),
               (MOP_MUL, 0, 1, 4), (MOP_I2F, 1, 0, 5), (MOP_LT, 3, 1, 6)]


@pytest.mark.gpu
@pytest.mark.parametrize("filter_reg", [-1, 6], ids=["nofilter", "filter"])
def test_device_surface_matches_reference(hip, filter_reg):
    from arroyo_amd import gpu
    rng = np.random.default_rng(5)
    n = 1061
    cols = [np.concatenate([rng.integers(I64_MIN, I64_MAX, size=n - len(EI),
                                         endpoint=True), EI]).astype(np.int64),
            rng.integers(-50, 50, size=n).astype(np.int64)]
    cfg = (2, DEVICE_PROG, [4, 5, 3, 0], filter_reg)
    want = ref_eval(cfg, [c.tolist() for c in cols])
    assert filter_reg < 0 or 0 < len(want[0]) < n
    op = gpu.make_map_op(make_cfg(cfg))
    got = device_run(hip, op, cols)
    # zero rows: nothing survives, nothing faults
    empty = device_run(hip, op, [cols[0][:0], cols[1][:0]])
    op.close()
    assert [len(c) for c in empty] == [0, 0, 0, 0]
    assert_cols(got, want)


@pytest.mark.gpu
def test_device_surface_rejects_bad_batches(hip):
    from arroyo_amd import gpu
    op = gpu.make_map_op(make_cfg((2, DEVICE_PROG, [4], 6)))
    d = hip.upload([1, 2, 3])
    with pytest.raises(RuntimeError, match="exceeds capacity"):
        op.process_batch_device([d, d], CHUNK + 1)
    with pytest.raises(RuntimeError, match="expected 2 cols"):
        op.process_batch_device([d], 3)
    with pytest.raises(RuntimeError, match="expected 2 cols"):
        op.process_batch_device([d, d, d], 3)
    op.close()


@pytest.mark.gpu
def test_device_surface_recovers_after_an_error(hip):
    from arroyo_amd import gpu
    cfg = binary(MOP_DIV)
    op = gpu.make_map_op(make_cfg(cfg))
    with pytest.raises(RuntimeError, match="division by zero"):
        device_run(hip, op, i64_cols([[1, 2, 3], [1, 0, 1]]))
    cols = [[7, -7, 9, I64_MIN], [2, 2, -3, 1]]
    got = device_run(hip, op, i64_cols(cols))
    op.close()
    assert_cols(got, ref_eval(cfg, cols))
    assert got[0].tolist() == [3, -3, -3, I64_MIN]


# ----------------------------------------------------------------- validation

K = MOP_CONST
# (what, rejected config, its minimal accepted neighbour); a config is
# (n_in_cols, prog, out_reg, filter_reg)
VALIDATION = [
    ("opcode above FDIV",
     (1, [(MOP_FDIV + 1, 0, 0, 1)], [0], -1),
     (1, [(MOP_FDIV, 0, 0, 1)], [0], -1)),
    ("opcode 99",
     (1, [(99, 0, 0, 1)], [1], -1), (1, [(MOP_NOT, 0, 0, 1)], [1], -1)),
    ("opcode below CONST",
     (1, [(-1, 0, 0, 1)], [0], -1), (1, [(K, 0, 0, 1)], [0], -1)),
    ("out_reg past the register file",
     (1, [(K, 0, 0, 31)], [32], -1), (1, [(K, 0, 0, 31)], [31], -1)),
    ("negative out_reg",
     (1, [], [-1], -1), (1, [], [0], -1)),
    ("out_reg never written",
     (2, [], [2], -1), (2, [], [1], -1)),
    ("second out_reg never written",
     (2, [(K, 0, 0, 4)], [4, 3], -1), (2, [(K, 0, 0, 4)], [4, 4], -1)),
    ("filter_reg below -1",
     (1, [], [0], -7), (1, [], [0], -1)),
    ("filter_reg -2",
     (1, [], [0], -2), (1, [], [0], 0)),
    ("filter_reg past the register file",
     (1, [(K, 0, 0, 31)], [0], 32), (1, [(K, 0, 0, 31)], [0], 31)),
    ("filter_reg never written",
     (2, [], [0], 2), (2, [], [0], 1)),
    ("binary op reads an unwritten a",
     (1, [(MOP_ADD, 5, 0, 5)], [5], -1),
     (1, [(K, 0, 0, 5), (MOP_ADD, 5, 0, 5)], [5], -1)),
    ("binary op reads an unwritten b",
     (1, [(MOP_FADD, 0, 5, 6)], [6], -1), (1, [(MOP_FADD, 0, 0, 6)], [6], -1)),
    ("register written only by a later instruction",
     (1, [(MOP_ADD, 0, 3, 4), (K, 0, 0, 3)], [4], -1),
     (1, [(K, 0, 0, 3), (MOP_ADD, 0, 3, 4)], [4], -1)),
    ("NOT reads an unwritten a (its b is not read)",
     (1, [(MOP_NOT, 7, 0, 1)], [1], -1), (1, [(MOP_NOT, 0, 7, 1)], [1], -1)),
    ("I2F reads an unwritten a (its b is not read)",
     (1, [(MOP_I2F, 7, 0, 1)], [1], -1), (1, [(MOP_I2F, 0, 7, 1)], [1], -1)),
    ("F2I reads an unwritten a (its b is not read)",
     (1, [(MOP_F2I, 7, 0, 1)], [1], -1), (1, [(MOP_F2I, 0, 7, 1)], [1], -1)),
    ("unread operand of CONST still range-checked",
     (1, [(K, 32, 0, 1)], [1], -1), (1, [(K, 31, 31, 1)], [1], -1)),
    ("unread b of NOT still range-checked",
     (1, [(MOP_NOT, 0, -1, 1)], [1], -1), (1, [(MOP_NOT, 0, 31, 1)], [1], -1)),
    ("dst past the register file",
     (1, [(K, 0, 0, 32)], [0], -1), (1, [(K, 0, 0, 31)], [0], -1)),
]


@pytest.mark.parametrize("what,bad,good", VALIDATION,
                         ids=[v[0].replace(" ", "_") for v in VALIDATION])
def test_create_validation(mod, what, bad, good):
    with pytest.raises(RuntimeError, match="invalid map"):
        mod.make_map_op(make_cfg(bad))
    op = mod.make_map_op(make_cfg(good))
    out = op.process_batch(i64_cols([[1, 2]] * good[0]))
    op.close()
    assert len(out) == len(good[2])


def test_oracle_accepts_more_than_six_outputs():
    op = oracle.make_map_op(make_cfg((1, [], [0] * 7, -1)))
    assert len(op.process_batch(i64_cols([[4, 5]]))) == 7
    op.close()


@pytest.mark.gpu
def test_hip_rejects_seven_outputs_loudly():
    from arroyo_amd import gpu
    with pytest.raises(RuntimeError, match="n_out <= 6"):
        gpu.make_map_op(make_cfg((1, [], [0] * 7, -1)))
    gpu.make_map_op(make_cfg((1, [], [0] * 6, -1))).close()
