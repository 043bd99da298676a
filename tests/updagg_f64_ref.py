"""Python model of the updating aggregate over Float64 value columns
(AmdUpdatingConfig.val_is_f64), independent of the kernels: the checker of
tests/test_updagg_f64.py and tests/test_updagg_f64_pipeline.py.  The C oracle
does not read the flags.

The rules are restated from DataFusion 48 and arrow-arith (restated, not
golden-pinned; see include/arroyo_amd_types.h).  Per key the model keeps the
live multiset of rows, None standing for a NULL cell, every cell as the raw
i64 plane word (an f64 column's words are bit patterns):

  SUM / AVG over an f64 column: math.fsum over all signed terms since the
      key's last reset (the flush or expire that found it empty), with the
      term count T and A = sum |x| for the error bound T * 2**-52 * A
  MIN / MAX / MEDIAN and the retractable forms: IEEE totalOrder on the bit
      patterns; an even-count median is (lo + hi) / 2.0 in binary64
  moments and co-moments: exact fractions.Fraction sums over the live rows,
      then the kernels' final formulas in binary64
  NULLs: the rule of tests/test_null_aggs.py -- an aggregate skips rows
      whose argument is NULL, COUNT / COUNT DISTINCT / REGR_COUNT are never
      NULL, every other aggregate is NULL without a contributing row or
      where its result is undefined.

An expected value is a Val: kind "i" (an integer, exact), "b" (an f64 bit
pattern, exact), "n" (some NaN), "s" (an f64 within `bound` of `value`) or
"m" (an f64 moment final, rtol = atol = 1e-9), or None for NULL."""
import math
import struct
from collections import Counter, namedtuple
from fractions import Fraction

import numpy as np

from arroyo_amd import cabi as C

COMOMENT = tuple(range(C.COVAR_POP, C.REGR_SXY + 1))
MOMENT = (C.STDDEV, C.STDDEV_POP, C.VAR, C.VAR_POP)
SAMPLE = (C.STDDEV, C.VAR, C.COVAR_SAMP)
ORDERED = (C.MIN, C.MAX, C.MIN_RETRACT, C.MAX_RETRACT, C.MEDIAN)

Val = namedtuple("Val", "kind value bound", defaults=(0.0,))

M64 = (1 << 64) - 1


def bits_of(x):
    """binary64 -> its bit pattern as an unsigned integer."""
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def f64_of(bits):
    """A bit pattern (signed or unsigned integer) -> binary64."""
    return struct.unpack("<d", struct.pack("<Q", int(bits) & M64))[0]


def plane(xs):
    """Floats or unsigned bit patterns -> the i64 plane an f64 column
    travels in."""
    words = [x if isinstance(x, int) else bits_of(x) for x in xs]
    return np.array(words, dtype=np.uint64).view(np.int64)


def total_order_key(bits):
    """IEEE 754 totalOrder as a sort key on the bit pattern: negatives
    below positives, negatives by falling magnitude, positives by rising
    magnitude; NaNs order by sign and payload like everything else."""
    bits = int(bits) & M64
    mag = bits & ((1 << 63) - 1)
    return (0, -mag) if bits >> 63 else (1, mag)


def median_bits(words):
    """MEDIAN over f64 bit patterns: Val "b" for a stored element, and for
    an even count the two-operation midpoint (Val "n" when that is a NaN,
    whose payload is the adder's business)."""
    xs = sorted((int(w) & M64 for w in words), key=total_order_key)
    w = len(xs)
    if w & 1:
        return Val("b", xs[w // 2])
    lo, hi = f64_of(xs[(w - 1) // 2]), f64_of(xs[w // 2])
    m = (lo + hi) / 2.0
    return Val("n", None) if math.isnan(m) else Val("b", bits_of(m))


def trunc_median(xs):
    xs = sorted(xs)
    w = len(xs)
    if w & 1:
        return xs[w // 2]
    t = xs[(w - 1) // 2] + xs[w // 2]
    return (abs(t) // 2) * (1 if t >= 0 else -1)


def _sqrt(x):
    return math.sqrt(x) if x >= 0 else math.nan


def moment_final(op, n, sx, sxx):
    """The kernel's final formulas (ueval_slot) on exact sums; None = NULL
    under null semantics, NaN otherwise."""
    mean = sx / n
    m2 = max(sxx - n * mean * mean, 0.0)
    samp = op in (C.STDDEV, C.VAR)
    if samp and n <= 1:
        return None
    var = m2 / (n - 1) if samp else m2 / n
    return _sqrt(var) if op in (C.STDDEV, C.STDDEV_POP) else var


def comoment_final(op, n, w):
    sy, sx, sxy, syy, sxx = w
    my, mx = sy / n, sx / n
    Sxy = sxy - n * mx * my
    Syy = max(syy - n * my * my, 0.0)
    Sxx = max(sxx - n * mx * mx, 0.0)
    if op == C.COVAR_POP:
        return Sxy / n
    if op == C.COVAR_SAMP:
        return Sxy / (n - 1) if n > 1 else None
    if op == C.CORR:
        return (Sxy / math.sqrt(Sxx * Syy)
                if n > 1 and Sxx > 0 and Syy > 0 else None)
    if op == C.REGR_SLOPE:
        return Sxy / Sxx if Sxx > 0 else None
    if op == C.REGR_INTERCEPT:
        return my - (Sxy / Sxx) * mx if Sxx > 0 else None
    if op == C.REGR_R2:
        if Sxx <= 0:
            return None
        return 1.0 if Syy <= 0 else (Sxy * Sxy) / (Sxx * Syy)
    return {C.REGR_AVGX: mx, C.REGR_AVGY: my, C.REGR_SXX: Sxx,
            C.REGR_SYY: Syy, C.REGR_SXY: Sxy}[op]


class RefF64UpdAgg:
    """process / flush / expire in the operators' shape.  flush() and
    expire() return the expected state {key: (Val-or-None per aggregate)}
    of the keys that are live afterwards; the emitted stream itself is not
    modelled, because whether an inexact sum changed between two flushes is
    the adder's business."""

    def __init__(self, cfg):
        self.n_keys = cfg.n_keys
        self.n_vals = cfg.n_value_cols
        self.ns = bool(cfg.null_semantics)
        self.isf = [bool(cfg.val_is_f64[c]) for c in range(8)]
        self.aggs = [(cfg.agg_ops[i], cfg.agg_col[i], cfg.agg_col2[i])
                     for i in range(cfg.n_aggs)]
        self.live = {}
        self.rows = {}
        self.terms = {}      # (key, col) -> signed f64 terms since the reset
        self.touch = {}
        self.epoch = 1

    # ---- ingest
    def process_batch_nullable(self, cols, valid):
        cols = [np.asarray(c).view(np.int64) for c in cols]
        n = len(cols[0])
        if valid is None:
            valid = [None] * len(cols)
        retr = cols[self.n_keys + self.n_vals]
        fcols = sorted({col for op, col, _ in self.aggs
                        if op in (C.SUM, C.AVG) and col >= 0
                        and self.isf[col]})
        for r in range(n):
            key = int(cols[0][r]) if self.n_keys else 0
            row = []
            for c in range(self.n_vals):
                m = valid[self.n_keys + c]
                ok = m is None or bool(m[r])
                row.append(int(cols[self.n_keys + c][r]) if ok else None)
            row = tuple(row)
            d = -1 if retr[r] else 1
            ms = self.live.setdefault(key, Counter())
            ms[row] += d
            if ms[row] == 0:
                del ms[row]
            for c in fcols:
                if row[c] is not None:
                    self.terms.setdefault((key, c), []).append(
                        d * f64_of(row[c]))
            self.rows[key] = self.rows.get(key, 0) + d
            self.touch[key] = self.epoch

    def process_batch(self, cols):
        self.process_batch_nullable(cols, None)

    # ---- evaluation
    def _args(self, key, col, col2=-1):
        out = []
        for row, k in self.live[key].items():
            assert k > 0, "retraction without a matching append"
            if row[col] is None or (col2 >= 0 and row[col2] is None):
                continue
            out += [row[col] if col2 < 0 else (row[col], row[col2])] * k
        return out

    def _num(self, col, word):
        """An argument as an exact Fraction, per its column's flag."""
        return Fraction(f64_of(word)) if self.isf[col] else Fraction(word)

    def _null(self):
        """No contributing row / undefined: NULL under null semantics, the
        NaN filler without."""
        return None if self.ns else Val("n", None)

    def _eval_one(self, key, op, col, col2):
        if op == C.COUNT and col < 0:
            return Val("i", self.rows[key])
        if op in COMOMENT:
            pairs = self._args(key, col, col2)
            n = len(pairs)
            if op == C.REGR_COUNT:
                return Val("i", n)
            if n == 0:
                return self._null()
            ys = [self._num(col, p[0]) for p in pairs]
            xs = [self._num(col2, p[1]) for p in pairs]
            w = (sum(ys), sum(xs), sum(x * y for x, y in zip(xs, ys)),
                 sum(y * y for y in ys), sum(x * x for x in xs))
            v = comoment_final(op, n, tuple(float(s) for s in w))
            return self._null() if v is None else Val("m", v)
        xs = self._args(key, col)
        n = len(xs)
        if op == C.COUNT:
            return Val("i", n)
        if op == C.COUNT_DISTINCT:
            return Val("i", len(set(xs)))      # identity by raw bits
        if n == 0:
            assert self.ns, "every row contributes without NULLs"
            return None
        f = self.isf[col]
        if op in MOMENT:
            q = [self._num(col, x) for x in xs]
            v = moment_final(op, n, float(sum(q)),
                             float(sum(x * x for x in q)))
            return self._null() if v is None else Val("m", v)
        if op in (C.SUM, C.AVG) and f:
            t = self.terms.get((key, col), [])
            s = math.fsum(t)
            bound = len(t) * 2.0 ** -52 * math.fsum(abs(x) for x in t)
            if op == C.SUM:
                return Val("s", s, bound)
            avg = s / n
            return Val("s", avg, bound / n + 2.0 ** -52 * abs(avg))
        if op == C.SUM:
            return Val("i", sum(xs))
        if op == C.AVG:
            return Val("m", sum(xs) / n)
        if op in ORDERED and f:
            if op == C.MEDIAN:
                return median_bits(xs)
            s = sorted((x & M64 for x in xs), key=total_order_key)
            return Val("b", s[0] if op in (C.MIN, C.MIN_RETRACT) else s[-1])
        if op in (C.MIN, C.MIN_RETRACT):
            return Val("i", min(xs))
        if op in (C.MAX, C.MAX_RETRACT):
            return Val("i", max(xs))
        if op == C.MEDIAN:
            return Val("i", trunc_median(xs))
        raise ValueError(f"model has no op {op}")

    def state(self):
        return {key: tuple(self._eval_one(key, *a) for a in self.aggs)
                for key, rows in self.rows.items() if rows > 0}

    def _reset(self, key):
        for k in [k for k in self.terms if k[0] == key]:
            del self.terms[k]

    def flush(self):
        for key, e in self.touch.items():
            if e == self.epoch and self.rows[key] == 0:
                self._reset(key)
        self.epoch += 1
        return self.state()

    def expire(self, idle):
        for key in self.touch:
            if self.epoch - self.touch[key] <= idle:
                continue
            self.rows[key] = 0
            self.live[key] = Counter()
            self._reset(key)
        return self.state()


def assert_val(got_word, got_valid, want, what=""):
    """One emitted cell (raw i64 plane word, validity) against a Val."""
    if want is None:
        assert not got_valid, f"{what}: want NULL"
        assert got_word == 0, f"{what}: value under a NULL is {got_word}"
        return
    assert got_valid, f"{what}: NULL, want {want}"
    g = f64_of(got_word)
    if want.kind == "i":
        assert got_word == want.value, (what, got_word, want.value)
    elif want.kind == "b":
        assert got_word & M64 == want.value, \
            (what, hex(got_word & M64), hex(want.value), g,
             f64_of(want.value))
    elif want.kind == "n":
        assert math.isnan(g), (what, g)
    elif want.kind == "s":
        err = abs(g - want.value)
        print(f"{what}: got {g!r} fsum {want.value!r} err {err:.3e} "
              f"bound {want.bound:.3e}")
        assert err <= want.bound, (what, g, want.value, err, want.bound)
    else:
        np.testing.assert_allclose(g, want.value, rtol=1e-9, atol=1e-9,
                                   err_msg=what)
