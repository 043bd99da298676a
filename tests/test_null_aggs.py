"""SQL NULL semantics in the updating aggregate (null_semantics = 1): Arrow
validity bitmaps on the value columns in, validity bitmaps on the aggregate
columns out.

The C oracle has no NULLs, so the expected values come from RefNullUpdAgg
below, a pure-Python model in the shape of RefUpdAgg (tests/
test_ordered_aggs.py).  Per key it holds the live multiset of rows with None
for NULL and applies DataFusion's accumulator rule, which is what the
reference's IncrementalAggregatingFunc runs per key
(crates/arroyo-worker/src/arrow/incremental_aggregator.rs): an aggregate
skips rows whose argument is NULL (either argument for the two-argument
family), COUNT / COUNT DISTINCT / REGR_COUNT are never NULL, and every other
aggregate is NULL when no contributing row is left or its result is undefined
(sample variants over fewer than two rows, zero-variance CORR / REGR_SLOPE /
REGR_INTERCEPT / REGR_R2).  f64 finals are computed with numpy over the
non-null values.

CPU tests pin the model on hand-written cases and on the reference's
every_aggregate golden before the GPU is compared with the model."""
import ctypes
import functools
from collections import Counter

import numpy as np
import pytest

from arroyo_amd import cabi
from tests.golden_util import load_golden, load_inputs

C = cabi
ONE_ARG_F64 = (C.AVG, C.STDDEV, C.STDDEV_POP, C.VAR, C.VAR_POP)
COMOMENT = tuple(range(C.COVAR_POP, C.REGR_SXY + 1))
SAMPLE = (C.STDDEV, C.VAR, C.COVAR_SAMP)
NEVER_NULL = (C.COUNT, C.COUNT_DISTINCT, C.REGR_COUNT)
# a value stored under a NULL input cell: must never reach an aggregate
GARBAGE = 7_777_777


def i64(x):
    return np.array(x, dtype=np.int64)


def is_f64_op(op):
    return op in ONE_ARG_F64 or (op in COMOMENT and op != C.REGR_COUNT)


def trunc_median(xs):
    """DataFusion's integer median: middle element, or (lo + hi) / 2
    truncated toward zero."""
    xs = sorted(xs)
    w = len(xs)
    if w & 1:
        return xs[w // 2]
    t = xs[(w - 1) // 2] + xs[w // 2]
    return (abs(t) // 2) * (1 if t >= 0 else -1)


class RefNullUpdAgg:
    """Model with the operators' process / flush / expire shape.  `live`
    maps key -> Counter of row tuples (None = NULL).  Emitted rows are
    (key?, value-or-None per aggregate..., is_retract).  `hits` records
    which interesting cases a run went through."""

    def __init__(self, cfg):
        self.n_keys = cfg.n_keys
        self.n_vals = cfg.n_value_cols
        self.aggs = [(cfg.agg_ops[i], cfg.agg_col[i], cfg.agg_col2[i])
                     for i in range(cfg.n_aggs)]
        self.live = {}
        self.rows = {}
        self.last = {}
        self.touch = {}
        self.epoch = 1
        self.hits = set()

    def process_batch_nullable(self, cols, valid):
        cols = [np.asarray(c, dtype=np.int64) for c in cols]
        n = len(cols[0])
        if valid is None:
            valid = [None] * len(cols)
        retr = cols[self.n_keys + self.n_vals]
        for r in range(n):
            key = int(cols[0][r]) if self.n_keys else 0
            row = []
            for c in range(self.n_vals):
                m = valid[self.n_keys + c]
                ok = m is None or bool(m[r])
                row.append(int(cols[self.n_keys + c][r]) if ok else None)
            row = tuple(row)
            d = -1 if retr[r] else 1
            if d < 0 and any(op in (C.MIN, C.MAX) for op, _, _ in self.aggs):
                raise RuntimeError("MIN/MAX do not support retraction")
            ms = self.live.setdefault(key, Counter())
            ms[row] += d
            if ms[row] == 0:
                del ms[row]
            self.rows[key] = self.rows.get(key, 0) + d
            self.touch[key] = self.epoch

    def process_batch(self, cols):
        self.process_batch_nullable(cols, None)

    def _args(self, key, col, col2=-1):
        """The contributing rows' argument values, with multiplicity."""
        out = []
        for row, k in self.live[key].items():
            assert k > 0, "retraction without a matching append"
            if row[col] is None or (col2 >= 0 and row[col2] is None):
                continue
            out += [row[col] if col2 < 0 else (row[col], row[col2])] * k
        return sorted(out)

    def _eval_one(self, key, op, col, col2):
        if op == C.COUNT and col < 0:
            return self.rows[key]
        if op in COMOMENT:
            return self._eval_comoment(op, self._args(key, col, col2))
        xs = self._args(key, col)
        n = len(xs)
        if op == C.COUNT:
            return n
        if op == C.COUNT_DISTINCT:
            return len(set(xs))
        if n == 0:
            self.hits.add("all_null_live")
            return None
        if op in SAMPLE and n == 1:
            self.hits.add("sample_n1")
            return None
        a = np.array(xs, dtype=np.float64)
        if op == C.SUM:
            return sum(xs)
        if op == C.AVG:
            return float(np.float64(sum(xs)) / np.float64(n))
        if op in (C.MIN, C.MIN_RETRACT):
            return xs[0]
        if op in (C.MAX, C.MAX_RETRACT):
            return xs[-1]
        if op == C.MEDIAN:
            return trunc_median(xs)
        if op == C.STDDEV:
            return float(a.std(ddof=1))
        if op == C.STDDEV_POP:
            return float(a.std(ddof=0))
        if op == C.VAR:
            return float(a.var(ddof=1))
        if op == C.VAR_POP:
            return float(a.var(ddof=0))
        if op == C.BIT_XOR:
            return int(functools.reduce(lambda p, q: p ^ q, xs))
        if op == C.BIT_AND:
            return int(functools.reduce(lambda p, q: p & q, xs))
        if op == C.BIT_OR:
            return int(functools.reduce(lambda p, q: p | q, xs))
        raise ValueError(f"model has no op {op}")

    def _eval_comoment(self, op, pairs):
        n = len(pairs)
        if op == C.REGR_COUNT:
            return n
        if n == 0:
            self.hits.add("all_null_live")
            return None
        y = np.array([p[0] for p in pairs], dtype=np.float64)
        x = np.array([p[1] for p in pairs], dtype=np.float64)
        # zero variance is decided on the exact integer data
        x_const = len(set(p[1] for p in pairs)) == 1
        y_const = len(set(p[0] for p in pairs)) == 1
        my, mx = y.mean(), x.mean()
        Sxy = float(((x - mx) * (y - my)).sum())
        Sxx = float(((x - mx) ** 2).sum())
        Syy = float(((y - my) ** 2).sum())
        if op == C.COVAR_POP:
            return Sxy / n
        if op == C.COVAR_SAMP:
            if n < 2:
                self.hits.add("sample_n1")
                return None
            return Sxy / (n - 1)
        if op == C.CORR:
            if n < 2:
                self.hits.add("sample_n1")
                return None
            if x_const or y_const:
                return None
            return Sxy / float(np.sqrt(Sxx * Syy))
        if op in (C.REGR_SLOPE, C.REGR_INTERCEPT, C.REGR_R2):
            if x_const:
                return None
            if op == C.REGR_SLOPE:
                return Sxy / Sxx
            if op == C.REGR_INTERCEPT:
                return float(my - (Sxy / Sxx) * mx)
            return 1.0 if y_const else Sxy * Sxy / (Sxx * Syy)
        return {C.REGR_AVGX: float(mx), C.REGR_AVGY: float(my),
                C.REGR_SXX: Sxx, C.REGR_SYY: Syy, C.REGR_SXY: Sxy}[op]

    def _eval(self, key):
        return tuple(self._eval_one(key, *a) for a in self.aggs)

    def flush(self):
        out = []
        kp = (lambda k: (k,)) if self.n_keys else (lambda k: ())
        for key in sorted(k for k, e in self.touch.items()
                          if e == self.epoch):
            rows = self.rows[key]
            cur = self._eval(key) if rows > 0 else None
            if key in self.last:
                last = self.last[key]
                if cur == last:
                    continue
                if cur is not None:
                    for (op, _, _), lv, cv in zip(self.aggs, last, cur):
                        if lv is None and cv is not None:
                            self.hits.add("null_to_value")
                        if lv is not None and cv is None:
                            self.hits.add("value_to_null")
                out.append(kp(key) + last + (1,))
                del self.last[key]
                if cur is not None:
                    out.append(kp(key) + cur + (0,))
                    self.last[key] = cur
            elif cur is not None:
                out.append(kp(key) + cur + (0,))
                self.last[key] = cur
        self.epoch += 1
        return out

    def expire(self, idle):
        out = []
        kp = (lambda k: (k,)) if self.n_keys else (lambda k: ())
        for key in sorted(self.touch):
            if self.epoch - self.touch[key] <= idle:
                continue
            if key not in self.last and self.rows[key] == 0:
                continue
            if key in self.last:
                out.append(kp(key) + self.last.pop(key) + (1,))
            self.rows[key] = 0
            self.live[key] = Counter()
        return out

    def close(self):
        pass


# ------------------------------------------------------------ GPU adapters


def decode(cols, masks):
    """(cols, masks) of flush_with_validity -> row tuples with None for NULL.
    The value plane under a NULL must hold 0."""
    n = len(cols[0]) if cols else 0
    rows = []
    for r in range(n):
        row = []
        for c, m in zip(cols, masks):
            if m[r]:
                row.append(float(c[r]) if c.dtype == np.float64
                           else int(c[r]))
            else:
                assert c.view(np.int64)[r] == 0, "value under a NULL is not 0"
                row.append(None)
        rows.append(tuple(row))
    return rows


class GpuNull:
    """The GPU operator behind the model's interface."""

    def __init__(self, cfg):
        from arroyo_amd import gpu
        self.op = gpu.make_updagg_op(cfg)

    def process_batch_nullable(self, cols, valid):
        self.op.process_batch_nullable(cols, valid)

    def process_batch(self, cols):
        self.op.process_batch(cols)

    def flush(self):
        return decode(*self.op.flush_with_validity())

    def expire(self, idle):
        return decode(*self.op.expire_with_validity(idle))

    def close(self):
        self.op.close()


def fold(state, rows, n_keys=1):
    """Fold emitted rows into {key: values}; a retract must carry exactly
    the values (and NULLs) emitted before."""
    for row in rows:
        key, vals, retract = ((row[0], row[1:-1], row[-1]) if n_keys
                              else (0, row[:-1], row[-1]))
        if retract:
            assert state.get(key) == vals, f"retract of non-current {key}"
            del state[key]
        else:
            assert key not in state, f"append over live key {key}"
            state[key] = vals
    return state


def assert_state_close(got, want):
    """Integers and NULLs exactly, f64 with the tolerance of
    tests/test_moment_aggs.py."""
    assert set(got) == set(want)
    for k, w in want.items():
        g = got[k]
        assert len(g) == len(w)
        for i, (gv, wv) in enumerate(zip(g, w)):
            if wv is None or gv is None or isinstance(wv, int):
                assert gv == wv and type(gv) is type(wv), (k, i, gv, wv)
            else:
                np.testing.assert_allclose(gv, wv, rtol=1e-9, atol=1e-9,
                                           err_msg=f"key {k} agg {i}")


def int_projection(rows, aggs, n_keys=1):
    """Emitted rows without their f64 columns, sorted."""
    keep = list(range(n_keys)) + [n_keys + i for i, a in enumerate(aggs)
                                  if not is_f64_op(a[0])]
    keep.append(n_keys + len(aggs))
    return sorted((tuple(r[c] for c in keep) for r in rows),
                  key=lambda t: tuple((x is None, x or 0) for x in t))


def both(cfg_fn):
    return GpuNull(cfg_fn()), RefNullUpdAgg(cfg_fn())


def step(g, m, cols, valid, aggs, n_keys=1):
    """Feed one nullable batch to GPU and model, flush both, compare the
    emitted integer rows exactly; returns the model's rows."""
    g.process_batch_nullable(cols, valid)
    m.process_batch_nullable(cols, valid)
    got, want = g.flush(), m.flush()
    assert int_projection(got, aggs, n_keys) == \
        int_projection(want, aggs, n_keys)
    return got, want


# ------------------------------------------------------------ shared inputs

FUZZ_A = [(C.COUNT, -1), (C.COUNT, 0), (C.SUM, 0), (C.AVG, 0),
          (C.COUNT_DISTINCT, 0), (C.MEDIAN, 0), (C.MIN_RETRACT, 0),
          (C.MAX_RETRACT, 0)]
FUZZ_B = [(C.STDDEV, 0), (C.VAR_POP, 0), (C.BIT_AND, 0), (C.BIT_XOR, 0),
          (C.CORR, 0, 1), (C.REGR_COUNT, 0, 1)]
FUZZ_HITS = {"all_null_live", "null_to_value", "value_to_null"}
FUZZ_SEED = {"A": 2, "B": 2}


def fuzz_cfg(which):
    if which == "A":
        return cabi.make_updagg_config(FUZZ_A, n_keys=1, n_value_cols=1,
                                       null_semantics=True)
    return cabi.make_updagg_config(FUZZ_B, n_keys=1, n_value_cols=2,
                                   null_semantics=True)


@functools.lru_cache(maxsize=None)
def fuzz_stream(seed, n_vals, n=6000, n_keys=40):
    """About n rows over n_keys keys; 35% of the rows of a key with live
    rows retract one of them, 25% NULLs per value column (independent),
    values in [-50, 50) so f64 sums are exact.  Key frequencies fall off as
    1/(k+1)^2, so the stream holds busy keys as well as keys with a handful
    of rows -- the ones that pass through all-NULL, NULL -> value and
    value -> NULL."""
    rng = np.random.default_rng(seed)
    p = 1.0 / (np.arange(n_keys) + 1.0) ** 2
    key = rng.choice(n_keys, size=n, p=p / p.sum()).astype(np.int64)
    vals = [rng.integers(-50, 50, size=n).astype(np.int64)
            for _ in range(n_vals)]
    masks = [rng.random(n) >= 0.25 for _ in range(n_vals)]
    retract = np.zeros(n, dtype=np.int64)
    live = {}
    for i in range(n):
        k = int(key[i])
        if live.get(k) and rng.random() < 0.35:
            row = live[k].pop(int(rng.integers(0, len(live[k]))))
            retract[i] = 1
            for c in range(n_vals):
                masks[c][i] = row[c] is not None
                vals[c][i] = row[c] if row[c] is not None else 0
        else:
            live.setdefault(k, []).append(tuple(
                int(vals[c][i]) if masks[c][i] else None
                for c in range(n_vals)))
    for c in range(n_vals):
        vals[c][~masks[c]] = GARBAGE
    for a in [key, retract] + vals + masks:
        a.setflags(write=False)
    return key, vals, masks, retract


def run_fuzz(make_op, which, flushes=6):
    n_vals = 1 if which == "A" else 2
    key, vals, masks, retract = fuzz_stream(FUZZ_SEED[which], n_vals)
    op = make_op(fuzz_cfg(which))
    per_flush = []
    n = len(key)
    stp = n // flushes
    for b in range(0, n, stp):
        sl = slice(b, min(b + stp, n))
        op.process_batch_nullable(
            [key[sl]] + [v[sl] for v in vals] + [retract[sl]],
            [None] + [m[sl] for m in masks] + [None])
        per_flush.append(op.flush())
    hits = getattr(op, "hits", None)
    op.close()
    return per_flush, hits


@functools.lru_cache(maxsize=None)
def model_fuzz(which):
    return run_fuzz(RefNullUpdAgg, which)


def cfg1(aggs, n_keys=1, n_value_cols=1, **kw):
    return lambda: cabi.make_updagg_config(aggs, n_keys=n_keys,
                                           n_value_cols=n_value_cols,
                                           null_semantics=True, **kw)


# ---------------------------------------------------- CPU: pin the yardstick


def model_rows(aggs, batches, n_vals=1, n_keys=1):
    """batches: lists of (key, v0[, v1], retract) with None for NULL."""
    m = RefNullUpdAgg(cfg1(aggs, n_keys=n_keys, n_value_cols=n_vals)())
    out = []
    for rows in batches:
        cols = [i64([0 if x is None else x for x in col])
                for col in zip(*rows)]
        valid = [np.array([x is not None for x in col])
                 for col in zip(*rows)]
        m.process_batch_nullable(cols, valid)
        out.append(m.flush())
    return out


def test_model_all_null_key():
    aggs = [(C.COUNT, -1), (C.COUNT, 0), (C.SUM, 0), (C.AVG, 0),
            (C.MIN_RETRACT, 0), (C.COUNT_DISTINCT, 0)]
    out = model_rows(aggs, [[(1, None, 0)] * 3])
    assert out == [[(1, 3, 0, None, None, None, 0, 0)]]


def test_model_single_value_sample_vs_population():
    aggs = [(C.STDDEV, 0), (C.STDDEV_POP, 0), (C.VAR, 0), (C.VAR_POP, 0),
            (C.COUNT, 0)]
    out = model_rows(aggs, [[(1, 9, 0), (1, None, 0)]])
    assert out == [[(1, None, 0.0, None, 0.0, 1, 0)]]


def test_model_pairwise_nulls():
    aggs = [(C.REGR_COUNT, 0, 1), (C.REGR_AVGX, 0, 1), (C.REGR_AVGY, 0, 1),
            (C.COVAR_POP, 0, 1), (C.CORR, 0, 1), (C.REGR_SLOPE, 0, 1),
            (C.COUNT, 0), (C.COUNT, 1)]
    rows = [(1, 2, 10, 0), (1, 4, 20, 0), (1, None, 30, 0), (1, 6, None, 0),
            (1, None, None, 0)]
    (row,), = model_rows(aggs, [rows], n_vals=2)
    # only (2, 10) and (4, 20) are complete pairs: y = x / 5
    assert row[1] == 2 and row[2] == 15.0 and row[3] == 3.0
    assert row[4] == pytest.approx(5.0) and row[5] == pytest.approx(1.0)
    assert row[6] == pytest.approx(0.2)
    assert row[7] == 3 and row[8] == 3
    # one complete pair: sample/zero-variance results are NULL
    (row,), = model_rows(aggs, [rows[:1] + rows[2:]], n_vals=2)
    assert row[1:7] == (1, 10.0, 2.0, 0.0, None, None)


def test_model_null_arrives_then_retracts():
    aggs = [(C.COUNT, -1), (C.COUNT, 0), (C.SUM, 0)]
    out = model_rows(aggs, [
        [(1, 5, 0)],
        [(1, None, 0)],          # COUNT(*) moves, COUNT(col) / SUM do not
        [(1, None, 1)],          # the NULL row goes
        [(1, 5, 1), (1, None, 0)],   # value -> NULL while the key lives
        [(1, None, 1)]])         # key gone: retract only
    assert out == [
        [(1, 1, 1, 5, 0)],
        [(1, 1, 1, 5, 1), (1, 2, 1, 5, 0)],
        [(1, 2, 1, 5, 1), (1, 1, 1, 5, 0)],
        [(1, 1, 1, 5, 1), (1, 1, 0, None, 0)],
        [(1, 1, 0, None, 1)]]


def test_model_all_valid_reproduces_every_aggregate_golden():
    inp = load_inputs()["cars"]
    etype = i64(inp["event_type_id"])
    driver = i64(inp["driver_id"])
    names = inp["event_type_dict"]
    aggs = [(C.COUNT, -1), (C.MEDIAN, 0), (C.MIN_RETRACT, 0),
            (C.MAX_RETRACT, 0), (C.SUM, 0), (C.AVG, 0), (C.MIN, 0),
            (C.MAX, 0)]
    m = RefNullUpdAgg(cfg1(aggs)())
    m.process_batch([etype, driver, np.zeros(len(etype), dtype=np.int64)])
    state = {names[k]: v for k, v in fold({}, m.flush()).items()}
    want = {g["after"]["event_type"]: g["after"]
            for g in load_golden("every_aggregate")}
    assert set(state) == set(want) and len(want) == 2
    for et, (cnt, med, mn, mx, sm, avg, mn2, mx2) in state.items():
        w = want[et]
        assert (cnt, med, mn, mx, sm, mn2, mx2) == (
            w["cnt"], w["median_driver"], w["min_driver"], w["max_driver"],
            w["sum_driver"], w["min_driver"], w["max_driver"])
        assert round(avg, 4) == w["avg_driver"]


@pytest.mark.parametrize("n", [0, 1, 7, 8, 9, 63, 64, 65])
def test_pack_validity_roundtrip(n):
    rng = np.random.default_rng(n)
    mask = rng.random(n) < 0.5
    bm = cabi.pack_validity(mask)
    assert bm.dtype == np.uint8 and len(bm) == (n + 7) // 8
    for r in range(n):
        assert bool(bm[r >> 3] >> (r & 7) & 1) == bool(mask[r])
    if n % 8:
        assert bm[-1] >> (n % 8) == 0      # padding bits clear
    # through out_validity, the decoder of AmdOutBatch bitmaps
    keep = np.concatenate([bm, np.zeros(1, dtype=np.uint8)])
    ptr = keep.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
    tbl = (ctypes.POINTER(ctypes.c_uint8) * 2)(ptr, None)
    out = cabi.AmdOutBatch()
    out.n_rows, out.n_cols = n, 2
    out.validity = ctypes.cast(
        tbl, ctypes.POINTER(ctypes.POINTER(ctypes.c_uint8)))
    got = cabi.out_validity(out)
    assert got[1] is None
    assert np.array_equal(got[0], mask)


def test_config_null_semantics_field():
    fields = [f[0] for f in cabi.AmdUpdatingConfig._fields_]
    assert fields[-1] == "null_semantics"      # appended, not inserted
    old = type("Old", (ctypes.Structure,),
               {"_fields_": cabi.AmdUpdatingConfig._fields_[:-1]})
    assert ctypes.sizeof(cabi.AmdUpdatingConfig) == ctypes.sizeof(old) + 4
    aggs = [(C.COUNT, -1)]
    assert cabi.make_updagg_config(aggs).null_semantics == 0
    assert cabi.make_updagg_config(aggs, null_semantics=True) \
        .null_semantics == 1


@pytest.mark.parametrize("which", ["A", "B"])
def test_fuzz_stream_reaches_the_cases(which):
    """Precondition of the GPU fuzz, checkable without a GPU: the model's
    run passes through every case the comparison is meant to cover."""
    _, hits = model_fuzz(which)
    need = FUZZ_HITS | ({"sample_n1"} if which == "B" else set())
    assert need <= hits, need - hits


# ----------------------------------------------------------------- GPU


def flush_raw(op):
    """flush through the C ABI: (cols, raw bitmap bytes or None per col)."""
    out = cabi.AmdOutBatch()
    rc = op._fn["flush"](op._h, ctypes.byref(out))
    assert rc == 0, op._fn["last_error"](op._h).decode()
    cols = cabi._out_to_numpy(out)
    n = out.n_rows
    assert bool(out.validity), "null_semantics = 1 must set out->validity"
    raw = []
    for c in range(out.n_cols):
        bm = out.validity[c]
        raw.append(bytes(bytearray(bm[i] for i in range((n + 7) // 8)))
                   if bm else None)
    op._fn["free_out"](ctypes.byref(out))
    return cols, raw


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 7, 8, 9, 63, 64, 65, 127, 129])
def test_bitmap_addressing_gpu(n):
    from arroyo_amd import gpu
    aggs = [(C.COUNT, -1), (C.COUNT, 0), (C.SUM, 0), (C.MIN_RETRACT, 0)]
    nulls = sorted({0, n - 1} | {r for r in (63, 64) if r < n})
    key = np.arange(n, dtype=np.int64) + 1000
    val = (np.arange(n, dtype=np.int64) * 3) - 40
    mask = np.ones(n, dtype=bool)
    mask[nulls] = False
    val[~mask] = GARBAGE
    op = gpu.make_updagg_op(cfg1(aggs)())
    op.process_batch_nullable([key, val, np.zeros(n, dtype=np.int64)],
                              [None, mask, None])
    cols, raw = flush_raw(op)
    op.close()
    assert len(cols[0]) == n
    # key, COUNT(*), COUNT(col), is_retract: no bitmap
    assert raw[0] is None and raw[1] is None and raw[2] is None \
        and raw[5] is None
    assert raw[3] is not None and raw[4] is not None
    for c in (3, 4):
        bits = np.unpackbits(np.frombuffer(raw[c], dtype=np.uint8),
                             bitorder="little")
        assert len(raw[c]) == (n + 7) // 8
        assert not bits[n:].any(), "padding bits past n_rows must be 0"
        for r in range(n):
            src = int(cols[0][r]) - 1000
            assert bool(bits[r]) == bool(mask[src]), (c, r, src)
    for r in range(n):
        src = int(cols[0][r]) - 1000
        ok = bool(mask[src])
        want = (1, 1 if ok else 0, int(val[src]) if ok else 0,
                int(val[src]) if ok else 0, 0)
        assert tuple(int(cols[c][r]) for c in range(1, 6)) == want


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["A", "B"])
def test_null_fuzz_gpu_vs_model(which):
    aggs = FUZZ_A if which == "A" else FUZZ_B
    want, hits = model_fuzz(which)
    need = FUZZ_HITS | ({"sample_n1"} if which == "B" else set())
    assert need <= hits
    got, _ = run_fuzz(GpuNull, which)
    assert len(got) == len(want)
    gs, ws = {}, {}
    for g, w in zip(got, want):
        assert int_projection(g, aggs) == int_projection(w, aggs)
        assert_state_close(fold(gs, g), fold(ws, w))
    assert ws


@pytest.mark.gpu
def test_order_statistics_arena_path_with_nulls_gpu():
    """More than 256 distinct non-null values (the global-arena path of the
    select) plus NULL rows; then every non-null row is retracted: the order
    statistics become NULL, without an error and without a select."""
    aggs = [(C.COUNT, -1), (C.MEDIAN, 0), (C.MIN_RETRACT, 0),
            (C.MAX_RETRACT, 0), (C.COUNT_DISTINCT, 0)]
    g, m = both(cfg1(aggs))
    rng = np.random.default_rng(4)
    D, NN = 300, 20
    vals = rng.permutation(np.arange(-150, 150, dtype=np.int64) * 1001)
    assert len(np.unique(vals)) == D > 256
    val = np.concatenate([vals, np.full(NN, GARBAGE, dtype=np.int64)])
    mask = np.concatenate([np.ones(D, bool), np.zeros(NN, bool)])
    order = rng.permutation(D + NN)
    val, mask = val[order], mask[order]
    key = np.full(D + NN, 9, dtype=np.int64)
    zeros = np.zeros(D + NN, dtype=np.int64)
    _, want = step(g, m, [key, val, zeros], [None, mask, None], aggs)
    assert want == [(9, D + NN, -500, -150 * 1001, 149 * 1001, D, 0)]
    _, want = step(g, m, [key[:D], vals, np.ones(D, dtype=np.int64)],
                   None, aggs)
    assert want[-1] == (9, NN, None, None, None, 0, 0)
    # the key keeps working after it went NULL
    _, want = step(g, m, [i64([9, 9]), i64([4, 8]), i64([0, 0])], None, aggs)
    assert want[-1] == (9, NN + 2, 6, 4, 8, 2, 0)
    g.close()


@pytest.mark.gpu
def test_global_aggregate_null_value_null_gpu():
    aggs = [(C.COUNT, -1), (C.COUNT, 0), (C.SUM, 0), (C.MIN_RETRACT, 0)]
    g, m = both(cfg1(aggs, n_keys=0))
    T, F = np.array([True]), np.array([False])
    seq = [([i64([GARBAGE]), i64([0])], [F, None]),
           ([i64([5]), i64([0])], [T, None]),
           ([i64([5]), i64([1])], [T, None])]
    outs = [step(g, m, cols, valid, aggs, n_keys=0)[1]
            for cols, valid in seq]
    g.close()
    assert outs[0] == [(1, 0, None, None, 0)]
    assert outs[1] == [(1, 0, None, None, 1), (2, 1, 5, 5, 0)]
    assert outs[2] == [(2, 1, 5, 5, 1), (1, 0, None, None, 0)]


@pytest.mark.gpu
def test_append_only_min_max_nulls_gpu():
    aggs = [(C.MIN, 0), (C.MAX, 0), (C.COUNT, -1)]
    g, m = both(cfg1(aggs))
    key = i64([1, 1, 1, 2, 2])
    val = i64([GARBAGE, 7, -3, -GARBAGE, GARBAGE])
    mask = np.array([False, True, True, False, False])
    _, want = step(g, m, [key, val, np.zeros(5, dtype=np.int64)],
                   [None, mask, None], aggs)
    assert sorted(want) == [(1, -3, 7, 3, 0), (2, None, None, 2, 0)]
    # retracting a NULL is still a retraction on an append-only aggregate
    with pytest.raises(RuntimeError, match="retraction"):
        g.process_batch_nullable([i64([2]), i64([0]), i64([1])],
                                 [None, np.array([False]), None])
        g.flush()
    with pytest.raises(RuntimeError, match="retraction"):
        m.process_batch_nullable([i64([2]), i64([0]), i64([1])],
                                 [None, np.array([False]), None])
    g.close()


@pytest.mark.gpu
def test_host_chunk_boundary_gpu():
    """One batch of 2^20 + 9 rows crosses the host staging chunk: the second
    chunk's bitmap starts at byte 2^17 of the caller's.  The pure-Python
    model would need seconds for a million rows, so the expected values are
    its rule (count and sum the non-null values per key) in numpy."""
    from arroyo_amd import gpu
    n = (1 << 20) + 9
    rng = np.random.default_rng(6)
    key = rng.integers(0, 64, size=n).astype(np.int64)
    val = rng.integers(-1000, 1000, size=n).astype(np.int64)
    mask = np.ones(n, dtype=bool)
    mask[(1 << 20) - 8:(1 << 20) + 8] = False
    assert mask[(1 << 20) + 8] and not mask[(1 << 20) + 7]
    vin = np.where(mask, val, GARBAGE)
    aggs = [(C.COUNT, -1), (C.COUNT, 0), (C.SUM, 0)]
    op = gpu.make_updagg_op(cfg1(aggs)())
    op.process_batch_nullable([key, vin, np.zeros(n, dtype=np.int64)],
                              [None, mask, None])
    got = {r[0]: r[1:] for r in decode(*op.flush_with_validity())}
    op.close()
    want = {}
    for k in range(64):
        sel = key == k
        want[k] = (int(sel.sum()), int((sel & mask).sum()),
                   int(val[sel & mask].sum()), 0)
    assert got == want


@pytest.mark.gpu
def test_device_surface_equals_host_surface_gpu():
    import torch
    from arroyo_amd import gpu
    key, vals, masks, retract = fuzz_stream(59, 2, n=4000, n_keys=48)
    aggs = [(C.COUNT, -1), (C.COUNT, 0), (C.SUM, 1), (C.MEDIAN, 0),
            (C.BIT_XOR, 1), (C.REGR_COUNT, 0, 1)]
    mk = cfg1(aggs, n_value_cols=2)
    h, d = gpu.make_updagg_op(mk()), gpu.make_updagg_op(mk())
    dev = torch.device("cuda", 0)
    # 1000 rows: 125 bitmap bytes, padded to the 8-byte multiple the device
    # surface asks for
    for lo in range(0, 4000, 1000):
        sl = slice(lo, lo + 1000)
        cols = [key[sl], vals[0][sl], vals[1][sl], retract[sl]]
        h.process_batch_nullable(cols, [None, masks[0][sl], masks[1][sl],
                                        None])
        want = decode(*h.flush_with_validity())
        tcols = [torch.from_numpy(c.copy()).to(dev) for c in cols]
        tbm = []
        for m in masks:
            bm = np.zeros(128, dtype=np.uint8)
            bm[:125] = cabi.pack_validity(m[sl])
            tbm.append(torch.from_numpy(bm).to(dev))
        # fence torch's H2D stream before the op's stream reads the data
        torch.cuda.synchronize()
        d.process_batch_nullable_device(
            [t.data_ptr() for t in tcols],
            [None, tbm[0].data_ptr(), tbm[1].data_ptr(), None], 1000)
        got = decode(*d.flush_with_validity())
        assert int_projection(got, aggs) == int_projection(want, aggs)
        assert want
    h.close()
    d.close()


@pytest.mark.gpu
def test_checkpoint_roundtrip_with_null_emissions_gpu():
    from arroyo_amd import gpu
    key, vals, masks, retract = fuzz_stream(8, 1, n=3000, n_keys=40)
    aggs = [(C.COUNT, -1), (C.COUNT, 0), (C.SUM, 0), (C.MEDIAN, 0),
            (C.BIT_AND, 0)]
    mk = cfg1(aggs)
    mid = 1500
    feed = lambda op, sl: op.process_batch_nullable(
        [key[sl], vals[0][sl], retract[sl]], [None, masks[0][sl], None])
    a, ref = gpu.make_updagg_op(mk()), gpu.make_updagg_op(mk())
    for op in (a, ref):
        feed(op, slice(0, mid))
    e0 = decode(*a.flush_with_validity())
    assert sorted(decode(*ref.flush_with_validity()), key=repr) == \
        sorted(e0, key=repr)
    # some keys' last emission holds NULLs while they are live
    assert any(r[3] is None for r in e0)
    d0, d1 = a.checkpoint_drain(0), a.checkpoint_drain(1)
    a.close()
    # [key, rows, st words..., emitted, last..., last-emitted validity]
    sw = 2 + 2 + 2 + 2 + 33
    assert len(d0) == 1 + 1 + sw + 1 + len(aggs) + 1
    # COUNTs always valid; SUM / MEDIAN / BIT_AND of the one column are NULL
    # together; 0 = never emitted
    assert {0b00011} <= set(int(x) for x in d0[-1]) <= {0, 0b11111, 0b00011}
    b = gpu.make_updagg_op(mk())
    b.restore(0, d0)
    b.restore(1, d1)
    for op in (b, ref):
        feed(op, slice(mid, 3000))
    e1 = decode(*b.flush_with_validity())
    er = decode(*ref.flush_with_validity())
    b.close()
    ref.close()
    assert sorted(e1, key=repr) == sorted(er, key=repr)
    # the flush after the restore retracts rows that were emitted with NULLs
    assert any(r[-1] == 1 and r[3] is None for r in e1)
    # and the never-checkpointed operator agrees with the model
    m = RefNullUpdAgg(mk())
    feed(m, slice(0, mid))
    m0 = m.flush()
    feed(m, slice(mid, 3000))
    assert sorted(m0, key=repr) == sorted(e0, key=repr)
    assert sorted(m.flush(), key=repr) == sorted(er, key=repr)


@pytest.mark.gpu
def test_expire_reemits_last_validity_gpu():
    aggs = [(C.COUNT, -1), (C.SUM, 0), (C.MAX_RETRACT, 0)]
    g, m = both(cfg1(aggs))

    def feed(keys, vals_, retr):
        cols = [i64(keys), i64([GARBAGE if v is None else v for v in vals_]),
                i64(retr)]
        valid = [None, np.array([v is not None for v in vals_]), None]
        return step(g, m, cols, valid, aggs)[1]

    assert feed([1, 2, 2], [100, None, None], [0, 0, 0]) == \
        [(1, 1, 100, 100, 0), (2, 2, None, None, 0)]
    for v in (101, 102, 103):
        feed([1], [v], [0])
    got, want = g.expire(2), m.expire(2)
    g.close()
    assert got == want == [(2, 2, None, None, 1)]


@pytest.mark.gpu
def test_left_join_into_nullable_aggregate_gpu():
    """The composition the validity bitmaps exist for: updating LEFT join,
    then COUNT(*) / COUNT(right.col) / SUM(right.col) by key.  The join's
    output bitmap of the right value column feeds the aggregate; a late
    right match retracts a null-padded row."""
    from arroyo_amd import gpu
    HOUR, T0, NS = 3600 * 10**9, 1_600_000_000 * 10**9, 10**9
    join = gpu.make_expjoin_op(cabi.make_expjoin_config(
        24 * HOUR, n_left_vals=0, n_right_vals=1, join_type=cabi.JOIN_LEFT,
        updating=True))
    aggs = [(C.COUNT, -1), (C.COUNT, 0), (C.SUM, 0)]
    g, m = both(cfg1(aggs))
    a = i64
    batches = [
        (join.LEFT, [a([7, 8, 9]), a([0, 0, 0]), a([T0] * 3)]),
        (join.RIGHT, [a([7]), a([42]), a([0]), a([T0 + NS])]),
        (join.RIGHT, [a([8, 8]), a([5, 6]), a([0, 0]), a([T0 + 2 * NS] * 2)]),
        (join.RIGHT, [a([7]), a([42]), a([1]), a([T0 + 3 * NS])]),
    ]
    gs, ws = {}, {}
    saw_null_retract = False
    for side, cols in batches:
        keep, arr = cabi._cols_to_ptrs(cols)
        out = cabi.AmdOutBatch()
        rc = join._fn["process_batch"](join._h, side, arr, len(keep),
                                       len(keep[0]), ctypes.byref(out))
        assert rc == 0, join._fn["last_error"](join._h).decode()
        jc = cabi._out_to_numpy(out)
        jm = cabi.out_validity(out)
        join._fn["free_out"](ctypes.byref(out))
        # join output: [key, rval, ts, lp, rp, is_retract]
        assert jm[1] is not None and np.array_equal(jm[1], jc[4].astype(bool))
        saw_null_retract |= bool(((jc[5] == 1) & ~jm[1]).any())
        got, want = step(g, m, [jc[0], jc[1], jc[5]], [None, jm[1], None],
                         aggs)
        fold(gs, got)
        fold(ws, want)
        assert gs == ws
    join.close()
    g.close()
    assert saw_null_retract
    assert ws == {7: (1, 0, None), 8: (2, 2, 11), 9: (1, 0, None)}


class _Recording:
    """Adapts a null_semantics = 1 operator to the process_batch / flush
    interface of tests/test_moment_aggs.py's drivers, keeping the masks."""

    def __init__(self, op):
        self.op = op
        self.masks = []

    def process_batch(self, cols):
        self.op.process_batch(cols)    # legal on such a handle: all valid

    def flush(self):
        cols, masks = self.op.flush_with_validity()
        if len(cols[0]):
            self.masks.append(masks)
        return cols


@pytest.mark.gpu
def test_all_valid_input_equals_null_semantics_off_gpu():
    """null_semantics = 1 fed all-valid input emits what null_semantics = 0
    emits on the test_moment_aggs streams, with NULL exactly where the
    latter emits its NaN filler."""
    from arroyo_amd import gpu
    from tests import test_moment_aggs as tm
    # seeds under which the null_semantics = 0 run emits NaN fillers (the
    # co-moment driver's own seeds 9 and 10 never leave a key with one row)
    runs = [(tm.AGGS, 1, lambda op: tm.drive(op, seed=4)[0]),
            (tm.COV_AGGS_A, 2,
             lambda op: [o[0] for o in tm.cov_drive([op], seed=6)[0]
                         if len(o[0][0])])]
    for aggs, n_vals, drive in runs:
        off = gpu.make_updagg_op(cabi.make_updagg_config(
            aggs, n_keys=1, n_value_cols=n_vals))
        on = _Recording(gpu.make_updagg_op(cabi.make_updagg_config(
            aggs, n_keys=1, n_value_cols=n_vals, null_semantics=True)))
        e_off, e_on = drive(off), drive(on)
        off.close()
        on.op.close()
        assert len(e_off) == len(e_on) == len(on.masks) > 0
        nans = 0
        for co, cn, masks in zip(e_off, e_on, on.masks):
            o_ord = np.lexsort([co[-1], co[0]])
            n_ord = np.lexsort([cn[-1], cn[0]])
            for c, (x, y, mk) in enumerate(zip(co, cn, masks)):
                x, y, mk = x[o_ord], y[n_ord], mk[n_ord]
                assert x.dtype == y.dtype
                if x.dtype == np.float64:
                    nan = np.isnan(x)
                    nans += int(nan.sum())
                    assert np.array_equal(mk, ~nan), c
                    assert np.array_equal(x[~nan], y[~nan])
                    assert not y.view(np.int64)[nan].any()
                else:
                    assert mk.all() and np.array_equal(x, y)
        assert nans > 0


@pytest.mark.gpu
def test_nullable_errors_gpu():
    from arroyo_amd import gpu
    aggs = [(C.COUNT, -1), (C.SUM, 0)]
    cols = [i64([1]), i64([2]), i64([0])]
    T = np.array([True])
    off = gpu.make_updagg_op(cabi.make_updagg_config(aggs, n_keys=1,
                                                     n_value_cols=1))
    with pytest.raises(RuntimeError, match="null_semantics"):
        off.process_batch_nullable(cols, [None, T, None])
    with pytest.raises(RuntimeError, match="null_semantics"):
        off.process_batch_nullable_device([0, 0, 0], None, 0)
    off.close()
    on = gpu.make_updagg_op(cfg1(aggs)())
    with pytest.raises(RuntimeError, match="key column"):
        on.process_batch_nullable(cols, [T, None, None])
    with pytest.raises(RuntimeError, match="is_retract"):
        on.process_batch_nullable(cols, [None, None, T])
    with pytest.raises(RuntimeError, match="expected 3 cols, got 2"):
        on.process_batch_nullable(cols[:2], [None, T])
    # the operator is still usable, and untouched by the rejected calls
    on.process_batch_nullable(cols, [None, T, None])
    assert decode(*on.flush_with_validity()) == [(1, 1, 2, 0)]
    on.close()
