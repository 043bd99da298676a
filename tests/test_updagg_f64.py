"""Float64 value columns in the updating aggregate (val_is_f64): the GPU
operator against the Python model of tests/updagg_f64_ref.py.

The model's own rules are pinned first, without a GPU.  The GPU tests then
fold the emitted debezium stream into per-key state after every flush (a
retract must carry exactly the bits emitted before) and compare that state
with the model: integers, order statistics and the exact-class sums bit for
bit, general sums within the bound the model carries, moment finals at the
tolerance of tests/test_moment_aggs.py."""
import json
import lzma
import math
import os

import numpy as np
import pytest

from arroyo_amd import cabi
from tests import updagg_f64_ref as ref
from tests.updagg_f64_ref import Val, bits_of, f64_of, plane

C = cabi
HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "raw", "inputs",
                       "aggregate_updates.json.xz")

NEG_NAN = 0xFFF8000000000000
POS_NAN = 0x7FF8000000000000
ALL_ONES = 0xFFFFFFFFFFFFFFFF      # -NaN: encodes to the MAX identity 0
MAX_NAN = 0x7FFFFFFFFFFFFFFF       # +NaN: encodes to the MIN identity 0
SMALL = dict(log2_capacity=10, log2_nodes=13, log2_out_cap=12)


def i64(x):
    return np.array(x, dtype=np.int64)


def load_events():
    with lzma.open(FIXTURE, "rt") as f:
        return [json.loads(line) for line in f if line.strip()]


def event_rows(events):
    """c / u / d -> (row dict, is_retract): a u is a retract of `before`
    plus an append of `after`, a d a retract of `before`."""
    out = []
    for e in events:
        if e["op"] in ("u", "d"):
            out.append((e["before"], 1))
        if e["op"] in ("c", "u"):
            out.append((e["after"], 0))
    return out


# ------------------------------------------------------- the model, no GPU

def test_model_total_order():
    want = [NEG_NAN, bits_of(-math.inf), bits_of(-1.5), bits_of(-0.0),
            bits_of(0.0), bits_of(5e-324), bits_of(1.5), bits_of(math.inf),
            POS_NAN]
    rng = np.random.default_rng(3)
    for _ in range(5):
        mixed = [want[i] for i in rng.permutation(len(want))]
        assert sorted(mixed, key=ref.total_order_key) == want
    # NaNs order by payload, and the two identity collisions are the ends
    assert sorted([POS_NAN, MAX_NAN, ALL_ONES, NEG_NAN],
                  key=ref.total_order_key) == \
        [ALL_ONES, NEG_NAN, POS_NAN, MAX_NAN]


def test_model_median_rule():
    b = bits_of
    assert ref.median_bits([b(3.0), b(-1.0), b(2.0)]) == Val("b", b(2.0))
    assert ref.median_bits([b(1.0), b(2.5)]) == Val("b", b(1.75))
    assert ref.median_bits([b(0.0), b(-0.0)]) == Val("b", b(0.0))
    big = 1.7e308
    assert ref.median_bits([b(big), b(big)]) == Val("b", b(math.inf))
    assert ref.median_bits([b(big), b(1.0), b(-big), b(big)]) == \
        Val("b", b((1.0 + big) / 2.0))
    assert ref.median_bits([b(math.inf), b(-math.inf)]).kind == "n"
    assert ref.median_bits([POS_NAN, b(1.0)]).kind == "n"
    assert ref.median_bits([POS_NAN, b(1.0), b(2.0)]) == Val("b", b(2.0))


def test_model_fixture_live_multisets():
    """The debezium fixture's c / u / d stream through the model: 6
    products with 85-104 live rows each, and the model's aggregates equal a
    direct computation over the surviving orders."""
    events = load_events()
    assert len(events) == 830
    names = sorted({r["product_name"] for r, _ in event_rows(events)})
    assert len(names) == 6
    cfg = cabi.make_updagg_config(
        [(C.COUNT, -1), (C.SUM, 0), (C.MIN_RETRACT, 0), (C.MAX_RETRACT, 0),
         (C.MEDIAN, 0)], n_keys=1, n_value_cols=1, val_is_f64=(0,))
    m = ref.RefF64UpdAgg(cfg)
    rows = event_rows(events)
    m.process_batch([i64([names.index(r["product_name"]) for r, _ in rows]),
                     plane([float(r["price"]) for r, _ in rows]),
                     i64([d for _, d in rows])])
    state = m.flush()
    orders = {}
    for e in events:
        if e["op"] == "d":
            del orders[e["before"]["id"]]
        else:
            orders[e["after"]["id"]] = e["after"]
    assert len(state) == 6
    for k, name in enumerate(names):
        prices = sorted(float(o["price"]) for o in orders.values()
                        if o["product_name"] == name)
        n = len(prices)
        assert 85 <= n <= 104, (name, n)
        cnt, s, mn, mx, med = state[k]
        assert cnt == Val("i", n)
        assert abs(s.value - math.fsum(prices)) <= s.bound
        assert mn == Val("b", bits_of(prices[0]))
        assert mx == Val("b", bits_of(prices[-1]))
        mid = (prices[n // 2] if n & 1
               else (prices[n // 2 - 1] + prices[n // 2]) / 2.0)
        assert med == Val("b", bits_of(mid))


def test_config_val_is_f64_field():
    fields = [f[0] for f in cabi.AmdUpdatingConfig._fields_]
    assert fields[-2:] == ["val_is_f64", "null_semantics"]
    aggs = [(C.SUM, 0)]
    z = cabi.make_updagg_config(aggs, n_value_cols=2)
    assert list(z.val_is_f64) == [0] * 8
    f = cabi.make_updagg_config(aggs, n_value_cols=2, val_is_f64=(1,))
    assert list(f.val_is_f64) == [0, 1, 0, 0, 0, 0, 0, 0]


# ------------------------------------------------------------ GPU harness

class Gpu:
    """The GPU operator on the host or the device surface.  flush() and
    expire() return emitted rows as (key?, (word, valid)..., is_retract),
    every value as its raw i64 plane word."""

    def __init__(self, cfg, device=False):
        from arroyo_amd import gpu
        self.cfg = cfg
        self.op = gpu.make_updagg_op(cfg)
        self.device = device
        self.keep = []
        self.dtypes = None
        self.all_dtypes = []       # of every flush / expire batch

    def process(self, cols, valid=None):
        cols = [np.ascontiguousarray(np.asarray(c).view(np.int64))
                for c in cols]
        if not self.device:
            if self.cfg.null_semantics:
                self.op.process_batch_nullable(cols, valid)
            else:
                assert valid is None
                self.op.process_batch(cols)
            return
        import torch
        dev = torch.device("cuda", self.cfg.device)
        t = [torch.from_numpy(c.copy()).to(dev) for c in cols]
        vp = None
        if valid is not None:
            vp = []
            for m in valid:
                if m is None:
                    vp.append(None)
                    continue
                bm = np.zeros((len(m) + 63) // 64 * 8, dtype=np.uint8)
                bm[:(len(m) + 7) // 8] = cabi.pack_validity(m)
                t.append(torch.from_numpy(bm).to(dev))
                vp.append(t[-1].data_ptr())
        torch.cuda.synchronize()     # torch's copies before the op's stream
        self.keep.append(t)          # alive until the next flush has synced
        ptrs = [x.data_ptr() for x in t[:len(cols)]]
        if self.cfg.null_semantics:
            self.op.process_batch_nullable_device(ptrs, vp, len(cols[0]))
        else:
            self.op.process_batch_device(ptrs, len(cols[0]))

    def _rows(self, cols, masks):
        self.dtypes = [c.dtype for c in cols]
        self.all_dtypes.append(self.dtypes)
        words = [c.view(np.int64) for c in cols]
        nk = self.cfg.n_keys
        out = []
        for r in range(len(words[0]) if words else 0):
            row = [int(words[0][r])] if nk else []
            row += [(int(w[r]), bool(m[r]))
                    for w, m in zip(words[nk:-1], masks[nk:-1])]
            out.append(tuple(row) + (int(words[-1][r]),))
        return out

    def _emit(self, cols_masks):
        self.keep = []
        if self.cfg.null_semantics:
            return self._rows(*cols_masks)
        cols = cols_masks
        return self._rows(cols, [np.ones(len(c), dtype=bool) for c in cols])

    def flush(self):
        return self._emit(self.op.flush_with_validity()
                          if self.cfg.null_semantics else self.op.flush())

    def expire(self, idle):
        return self._emit(self.op.expire_with_validity(idle)
                          if self.cfg.null_semantics
                          else self.op.expire(idle))

    def close(self):
        self.op.close()


def fold(state, rows, n_keys=1):
    """Merge emitted rows into {key: cells}; a retract must carry exactly
    the cells emitted before."""
    for row in rows:
        key, cells, retract = ((row[0], row[1:-1], row[-1]) if n_keys
                               else (0, row[:-1], row[-1]))
        if retract:
            assert state.get(key) == cells, f"retract of non-current {key}"
            del state[key]
        else:
            assert key not in state, f"append over live key {key}"
            state[key] = cells
    return state


def check_state(got, want, exact_sums=False, what=""):
    assert set(got) == set(want), (what, sorted(got), sorted(want))
    for key, vals in want.items():
        for a, (cell, w) in enumerate(zip(got[key], vals)):
            if exact_sums and w is not None and w.kind == "s":
                w = Val("b", bits_of(w.value))
            ref.assert_val(cell[0], cell[1], w, f"{what} key {key} agg {a}")


def run_script(cfg_fn, script, device=False, exact_sums=False):
    """script: ("batch", cols[, valid]) / ("flush",) / ("expire", idle).
    The GPU state is compared with the model's after every flush and
    expire.  Returns (all emitted rows, final folded state, Gpu)."""
    g = Gpu(cfg_fn(), device)
    m = ref.RefF64UpdAgg(cfg_fn())
    nk = g.cfg.n_keys
    state, emitted = {}, []
    try:
        for i, step in enumerate(script):
            if step[0] == "batch":
                valid = step[2] if len(step) > 2 else None
                g.process(step[1], valid)
                m.process_batch_nullable(step[1], valid)
                continue
            if step[0] == "flush":
                rows, want = g.flush(), m.flush()
            else:
                rows, want = g.expire(step[1]), m.expire(step[1])
            emitted.append(rows)
            fold(state, rows, nk)
            check_state(state, want, exact_sums, f"step {i}")
    finally:
        g.close()
    return emitted, state, g


def exact_stream(rng, n, n_keys, scale, mag, n_cols=1, retract_frac=0.25):
    """n appends of integer multiples of 1/scale below mag, then retractions
    of a random quarter of them, shuffled so that every retraction follows
    its append.  Returns (key, [value columns as f64], is_retract)."""
    key = rng.integers(0, n_keys, size=n)
    vals = [rng.integers(-mag * scale + 1, mag * scale, size=n) / scale
            for _ in range(n_cols)]
    pick = rng.permutation(n)[:int(n * retract_frac)]
    pos = np.concatenate([np.arange(n) * 2, pick * 2 + 1
                          + 2 * rng.integers(0, n, size=len(pick))])
    order = np.argsort(pos, kind="stable")
    idx = np.concatenate([np.arange(n), pick])[order]
    retr = np.concatenate([np.zeros(n), np.ones(len(pick))])[order]
    return (i64(key[idx]), [v[idx] for v in vals], i64(retr))


def batches_of(key, vals, retr, sizes):
    """Split a stream into ("batch", ...) steps with a flush after each."""
    script, lo = [], 0
    for s in sizes:
        hi = min(lo + s, len(key))
        script.append(("batch", [key[lo:hi]] + [v[lo:hi] for v in vals]
                       + [retr[lo:hi]]))
        script.append(("flush",))
        lo = hi
    assert lo == len(key)
    return script


# ------------------------------------------------------------- GPU tests

@pytest.mark.gpu
def test_exact_sum_and_avg_are_bit_exact():
    """Multiples of 2**-10 below 2**20, at most 2**16 terms per key: every
    partial sum in any order fits 46 bits, so SUM is the model's fsum and
    AVG is sum / n, bit for bit.  The values are non-integers: reading the
    bits as integers fails loudly."""
    rng = np.random.default_rng(11)
    key, (v,), retr = exact_stream(rng, 3000, 5, 1024, 1 << 20)
    assert np.any(v != np.floor(v))
    cfg = lambda: cabi.make_updagg_config(
        [(C.SUM, 0), (C.AVG, 0), (C.COUNT, -1)], n_keys=1, n_value_cols=1,
        val_is_f64=(0,), **SMALL)
    run_script(cfg, batches_of(key, [plane(v)], retr, [1000, 1500, 1250]),
               exact_sums=True)


@pytest.mark.gpu
def test_exact_moments_and_mixed_comoments():
    """Multiples of 2**-4 up to 2**8, at most 2**12 terms per key: the sums
    of x, x*x and x*y are exact.  Column 0 and 2 are f64, column 1 is i64;
    one co-moment aggregate has an f64 Y and an i64 X, one the reverse."""
    rng = np.random.default_rng(12)
    key, (a, b, c), retr = exact_stream(rng, 2000, 4, 16, 1 << 8, n_cols=3)
    b = np.rint(b)                               # the i64 column
    cfg = lambda: cabi.make_updagg_config(
        [(C.STDDEV, 0), (C.STDDEV_POP, 0), (C.VAR, 2), (C.VAR_POP, 0),
         (C.COVAR_POP, 0, 1), (C.CORR, 0, 2), (C.REGR_SLOPE, 1, 0),
         (C.REGR_COUNT, 0, 1)], n_keys=1, n_value_cols=3,
        val_is_f64=(0, 2), **SMALL)
    emitted, _, g = run_script(
        cfg, batches_of(key, [plane(a), i64(b), plane(c)], retr,
                        [900, 800, 800]))
    assert g.dtypes[-2] == np.int64              # REGR_COUNT stays i64


def fixture_prices():
    return np.array([float(r["price"]) for r, _ in event_rows(load_events())
                     if r is not None])


@pytest.mark.gpu
@pytest.mark.parametrize("source", ["normal", "fixture"])
def test_general_sum_and_avg_within_bound(source):
    """|got - fsum| <= T * 2**-52 * sum|x| for a key with T terms since its
    last reset: twice the standard bound for T correctly rounded adds in
    any order or tree shape.  AVG: that bound / n + 2**-52 * |avg|."""
    rng = np.random.default_rng(13)
    n = 2400
    v = (rng.normal(100.0, 37.0, size=n) if source == "normal"
         else rng.choice(fixture_prices(), size=n))
    key = rng.integers(0, 6, size=n)
    # key 6 holds subnormals only: their sums are exact (multiples of
    # 2**-1074 below 2**-1022), so the bound holds only if the hardware add
    # keeps denormals
    sub = rng.permutation(n)[:64]
    key[sub] = 6
    v[sub] = rng.integers(1, 1000, size=64) * 5e-324 * rng.choice([-1, 1], 64)
    pick = rng.permutation(n)[:n // 4]
    key = i64(np.concatenate([key, key[pick]]))
    v = np.concatenate([v, v[pick]])
    retr = i64(np.concatenate([np.zeros(n), np.ones(len(pick))]))
    cfg = lambda: cabi.make_updagg_config(
        [(C.SUM, 0), (C.AVG, 0), (C.COUNT, -1)], n_keys=1, n_value_cols=1,
        val_is_f64=(0,), **SMALL)
    _, state, _ = run_script(
        cfg, batches_of(key, [plane(v)], retr, [1200, 1200, 600]))
    live = np.ones(len(v), dtype=bool)
    live[pick] = live[n:] = False
    want = math.fsum(v[live & (key == 6)])
    assert want != 0.0 and abs(want) < 2.0 ** -1022
    assert state[6][0] == (plane([want])[0], True)     # exact, not flushed


def order_cases():
    """key -> list of (bit pattern, is_retract) in stream order."""
    b = bits_of
    big = 1.7e308
    one = b(1.0)
    cases = {
        1: [b(-1.5), b(2.0), b(-3.25), b(7.0), b(0.5)],     # mixed signs
        2: [b(-0.0), b(0.0)],                  # lo = -0.0, hi = +0.0
        3: [b(-math.inf), b(1.0), b(math.inf)],
        4: [b(5e-324), b(-5e-324), b(1e-310), b(-2e-310)],  # subnormals
        5: [POS_NAN, NEG_NAN, b(1.0)],
        6: [ALL_ONES],                         # the MAX identity collision
        7: [MAX_NAN],                          # the MIN identity collision
        8: [one + k for k in range(10)],       # share all but the low byte
        9: [b(2.5), b(-2.5), b(2.5), b(-2.5)],  # differ in the top byte
        10: [b(big), b(big)],                  # lo + hi overflows to inf
        11: [b(1.0), b(4.0)],                  # lo != hi
        12: [b(math.inf), b(-math.inf)],       # inf - inf: a NaN median
        13: [ALL_ONES, MAX_NAN, b(0.0)],
    }
    stream = {k: [(w, 0) for w in ws] for k, ws in cases.items()}
    # appended and retracted in one batch; a retraction of the current max
    stream[14] = [(b(3.5), 0), (b(9.25), 0), (b(9.25), 1)]
    stream[15] = [(b(-7.0), 0), (b(8.0), 0), (b(8.0), 1), (b(-8.0), 0)]
    # chains of 255 / 256 / 257 distinct values: the LDS tile / arena seam
    for k, n in ((255, 255), (256, 256), (257, 257)):
        stream[k] = [(b((-1.0) ** i * (i + 0.5) * 1.25), 0)
                     for i in range(n)]
    return stream


def order_batches(stream, keys):
    key, val, retr = [], [], []
    for k in keys:
        for w, d in stream[k]:
            key.append(k)
            val.append(w)
            retr.append(d)
    return [i64(key), plane(val), i64(retr)]


@pytest.mark.gpu
def test_order_statistics_are_bit_exact():
    """MIN_RETRACT / MAX_RETRACT / MEDIAN under IEEE totalOrder, and the
    append-only MIN / MAX on the keys without a retraction."""
    stream = order_cases()
    cfg = lambda: cabi.make_updagg_config(
        [(C.MIN_RETRACT, 0), (C.MAX_RETRACT, 0), (C.MEDIAN, 0),
         (C.COUNT, -1)], n_keys=1, n_value_cols=1, val_is_f64=(0,), **SMALL)
    keys = sorted(stream)
    cols = order_batches(stream, keys)
    # second batch: retract one element of some keys, grow others
    b = bits_of
    more = {1: [(b(7.0), 1)], 3: [(b(1.0), 1)], 5: [(b(1.0), 1)],
            8: [(b(1.0) + 9, 1)], 10: [(b(1.7e308), 1), (b(-1.7e308), 0)],
            13: [(b(0.0), 1)], 256: [(b(1e300), 0)], 255: [(b(0.625), 1)]}
    _, state, g = run_script(
        cfg, [("batch", cols), ("flush",),
              ("batch", order_batches(more, sorted(more))), ("flush",)])
    assert [str(d) for d in g.dtypes] == \
        ["int64", "float64", "float64", "float64", "int64", "int64"]
    # spot checks against hand-written bits, independent of the model
    assert state[6] == ((ALL_ONES - (1 << 64), True),) * 3 + ((1, True),)
    assert state[7] == ((MAX_NAN, True),) * 3 + ((1, True),)
    assert state[2][2] == (b(0.0), True)
    assert state[11][2] == (b(2.5), True)

    append_only = [k for k in keys if all(d == 0 for _, d in stream[k])]
    cfg2 = lambda: cabi.make_updagg_config(
        [(C.MIN, 0), (C.MAX, 0)], n_keys=1, n_value_cols=1,
        val_is_f64=(0,), **SMALL)
    _, state2, g2 = run_script(
        cfg2, [("batch", order_batches(stream, append_only)), ("flush",)])
    assert state2[6] == ((ALL_ONES - (1 << 64), True),) * 2
    assert state2[7] == ((MAX_NAN, True),) * 2
    assert state2[1] == ((b(-3.25) - (1 << 64), True), (b(7.0), True))
    assert [str(d) for d in g2.dtypes] == ["int64", "float64", "float64",
                                           "int64"]


def residue_script(tail):
    one = lambda x, d: ("batch", [i64([7]), plane([x]), i64([d])])
    return [one(1e16, 0), one(1.0, 0), ("flush",), one(1e16, 1),
            one(1.0, 1)] + tail + [one(0.5, 0), ("flush",)]


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["flush", "expire"])
def test_deleted_key_leaves_no_residue(path):
    """1e16 + 1.0 - 1e16 - 1.0 leaves -1.0 in an f64 sum word.  The flush
    that finds the key empty must clear it: the key's next life starts from
    +0.0.  The expire variant cannot run the same four batches: a key
    without rows is always reset by the flush of the epoch that touched it,
    so no residue ever reaches expire.  What expire can leave behind is the
    state of a key that was evicted with rows live, here 1e16 + 1.0, so the
    variant checks that k_updagg_expire clears it (it zeroes every state
    word) and that the expire batch carries the dtypes of a flush batch."""
    cfg = lambda: cabi.make_updagg_config(
        [(C.SUM, 0), (C.AVG, 0), (C.VAR_POP, 0), (C.COVAR_POP, 0, 0)],
        n_keys=1, n_value_cols=1, val_is_f64=(0,), **SMALL)
    if path == "flush":
        emitted, state, _ = run_script(cfg, residue_script([("flush",)]))
        assert [r[-1] for r in emitted[1]] == [1]      # a retract only
    else:
        # the key goes idle with its rows live; other keys keep flushing
        other = ("batch", [i64([9]), plane([2.0]), i64([0])])
        script = residue_script([])[:3]
        script += [other, ("flush",)] * 3 + [("expire", 2)]
        script += residue_script([])[-2:]
        emitted, state, g = run_script(cfg, script)
        assert [(r[0], r[-1]) for r in emitted[4]] == [(7, 1)]
        assert [str(d) for d in g.all_dtypes[4]] == \
            ["int64"] + ["float64"] * 4 + ["int64"]
        assert all(d == g.all_dtypes[4] for d in g.all_dtypes)
    half = (bits_of(0.5), True)
    assert state[7] == (half, half, (0, True), (0, True))


def seam_expect(key, v, retr):
    """Per-key count, sum, min, max of an exact-class stream by integer
    arithmetic on v * 1024 (no retraction of a min or max is used)."""
    uk, inv = np.unique(key, return_inverse=True)
    d = 1 - 2 * retr
    q = np.rint(v * 1024).astype(np.int64)
    cnt = np.zeros(len(uk), dtype=np.int64)
    s = np.zeros(len(uk), dtype=np.int64)
    np.add.at(cnt, inv, d)
    np.add.at(s, inv, d * q)
    mn = np.full(len(uk), np.inf)
    mx = np.full(len(uk), -np.inf)
    np.minimum.at(mn, inv, v)
    np.maximum.at(mx, inv, v)
    s = s / 1024.0
    return uk, cnt, s, s / cnt, mn, mx


def seam_check(op, key, v):
    """Feed one batch, flush, and compare the final rows of the touched
    keys with seam_expect of everything fed so far."""
    op.process_batch([i64(key[-1]), plane_np(v[-1]),
                      np.zeros(len(key[-1]), dtype=np.int64)])
    out = op.flush()
    allk, allv = np.concatenate(key), np.concatenate(v)
    uk, cnt, s, avg, mn, mx = seam_expect(allk, allv,
                                          np.zeros(len(allk), np.int64))
    app = out[-1] == 0
    order = np.argsort(out[0][app])
    touched = np.isin(uk, key[-1])
    assert np.array_equal(out[0][app][order], uk[touched])
    for got, want in zip(out[1:-1], (s, avg, mn, mx, cnt)):
        assert got.dtype == want.dtype
        assert np.array_equal(got[app][order].view(np.int64),
                              want[touched].view(np.int64))


def plane_np(v):
    return np.ascontiguousarray(v, dtype=np.float64).view(np.int64)


SEAM_AGGS = [(C.SUM, 0), (C.AVG, 0), (C.MIN, 0), (C.MAX, 0), (C.COUNT, -1)]
SEAM_SIZES = [63, 64, 65, 255, 256, 257, 2048 * 256 + 1]


@pytest.mark.gpu
@pytest.mark.parametrize("keys", ["one", "distinct"])
def test_launch_seams(keys):
    """Batches around the wave (64), the block (256) and one grid-stride
    wrap plus one row (2048 blocks x 256 + 1), all rows on one key and all
    rows on distinct keys.  Multiples of 2**-10 below 2**10: with at most
    2**20 terms per key every partial sum fits 40 bits, so sums are exact
    in any order."""
    from arroyo_amd import gpu
    rng = np.random.default_rng(14)
    op = gpu.make_updagg_op(cabi.make_updagg_config(
        SEAM_AGGS, n_keys=1, n_value_cols=1, val_is_f64=(0,),
        log2_capacity=20 if keys == "distinct" else 10, log2_nodes=10))
    ks, vs, base = [], [], 0
    try:
        for n in SEAM_SIZES:
            ks.append(np.arange(base, base + n) if keys == "distinct"
                      else np.full(n, 5))
            base += n
            vs.append(rng.integers(-(1 << 20) + 1, 1 << 20, size=n) / 1024)
            seam_check(op, ks, vs)
    finally:
        op.close()


@pytest.mark.gpu
def test_host_batch_across_the_staging_chunk():
    """One host batch of 2**20 + 1 rows: the last row rides in a second
    staging chunk."""
    from arroyo_amd import gpu
    rng = np.random.default_rng(15)
    n = (1 << 20) + 1
    op = gpu.make_updagg_op(cabi.make_updagg_config(
        SEAM_AGGS, n_keys=1, n_value_cols=1, val_is_f64=(0,),
        log2_capacity=10, log2_nodes=10, log2_out_cap=12))
    try:
        key = rng.integers(0, 64, size=n)
        key[-1] = 99                 # the second chunk's row has its own key
        seam_check(op, [key],
                   [rng.integers(-(1 << 20) + 1, 1 << 20, size=n) / 1024])
    finally:
        op.close()


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_null_semantics(device):
    """NULLs across a 64-row bitmap word seam, a key whose rows are all
    NULL (every aggregate NULL with value 0, COUNT(col) 0), and NaN as a
    value, not a NULL."""
    rng = np.random.default_rng(16)
    n = 200
    key = rng.integers(0, 3, size=n)
    v = rng.integers(-4000, 4000, size=n) / 8.0
    valid = np.ones(n, dtype=bool)
    valid[58:70] = False                      # across the word seam at 64
    valid[127:129] = False                    # and the one at 128
    key[60] = 0                               # key 0 holds a NULL row
    key[190:] = 8                             # the all-NULL key
    valid[190:] = False
    v[~valid] = 7777777.0                     # garbage under a NULL
    key[180], v[180] = 9, math.nan            # NaN is a value
    key[181], v[181] = 9, 1.0
    cfg = lambda: cabi.make_updagg_config(
        [(C.SUM, 0), (C.AVG, 0), (C.MIN_RETRACT, 0), (C.MAX_RETRACT, 0),
         (C.MEDIAN, 0), (C.COUNT, 0), (C.COUNT, -1)], n_keys=1,
        n_value_cols=1, val_is_f64=(0,), null_semantics=True, **SMALL)
    mask = [None, valid, None]
    # second batch: retract key 0's non-null rows, leaving it all-NULL too
    k0 = (key == 0) & valid
    script = [("batch", [i64(key), plane_np(v), np.zeros(n, np.int64)], mask),
              ("flush",),
              ("batch", [i64(key[k0]), plane_np(v[k0]),
                         np.ones(int(k0.sum()), np.int64)]),
              ("flush",)]
    # SUM / AVG over key 9 hold a NaN: kind "s" cannot bound it
    emitted, state, _ = run_script(
        lambda: cabi.make_updagg_config(
            [(C.MIN_RETRACT, 0), (C.MAX_RETRACT, 0), (C.MEDIAN, 0),
             (C.COUNT, 0)], n_keys=1, n_value_cols=1, val_is_f64=(0,),
            null_semantics=True, **SMALL), script, device)
    null = (0, False)
    assert state[8] == (null, null, null, (0, True))
    assert state[9][0] == (bits_of(1.0), True)
    assert state[9][1] == (bits_of(math.nan), True)     # +NaN is the max
    not9 = key != 9
    script[0] = ("batch", [i64(key[not9]), plane_np(v[not9]),
                           np.zeros(int(not9.sum()), np.int64)],
                 [None, valid[not9], None])
    emitted, state, _ = run_script(cfg, script, device, exact_sums=True)
    assert state[8] == (null,) * 5 + ((0, True), (10, True))
    assert state[0][:5] == (null,) * 5      # all-NULL after the retractions


@pytest.mark.gpu
def test_null_semantics_append_only_min_max():
    """The one-word MIN / MAX over a flagged column with null_semantics: an
    all-NULL key is NULL with value 0 (the zero state must not decode to
    its NaN), NaN is a value, and a NULL next to values is skipped."""
    key = i64([1, 1, 1, 2, 2, 3, 3, 3])
    v = np.array([7777777.0, 7777777.0, 7777777.0, -2.5, 7777777.0,
                  math.nan, 1.0, -0.0])
    valid = np.array([0, 0, 0, 1, 0, 1, 1, 1], dtype=bool)
    cfg = lambda: cabi.make_updagg_config(
        [(C.MIN, 0), (C.MAX, 0), (C.SUM, 0), (C.COUNT, 0)], n_keys=1,
        n_value_cols=1, val_is_f64=(0,), null_semantics=True, **SMALL)
    for device in (False, True):
        g = Gpu(cfg(), device)
        try:
            g.process([key, plane_np(v), np.zeros(8, np.int64)],
                      [None, valid, None])
            state = fold({}, g.flush())
        finally:
            g.close()
        null = (0, False)
        assert state[1] == (null, null, null, (0, True))
        m25 = (int(plane([-2.5])[0]), True)
        assert state[2] == (m25, m25, m25, (1, True))
        assert state[3][0] == (int(plane([-0.0])[0]), True)
        assert state[3][1] == (bits_of(math.nan), True)
        assert math.isnan(f64_of(state[3][2][0])) and state[3][3] == (3, True)
        assert [str(d) for d in g.dtypes] == \
            ["int64", "float64", "float64", "float64", "int64", "int64"]


MIXED_AGGS = [(C.SUM, 0), (C.SUM, 1), (C.MIN_RETRACT, 1), (C.MAX_RETRACT, 0),
              (C.AVG, 1), (C.MEDIAN, 0), (C.COUNT_DISTINCT, 0),
              (C.COUNT, -1)]


def mixed_stream(seed, n=1500):
    rng = np.random.default_rng(seed)
    key, (a, b), retr = exact_stream(rng, n, 6, 1024, 1 << 12, n_cols=2)
    return key, plane_np(a), i64(np.rint(b)), retr


def mixed_cfg():
    return cabi.make_updagg_config(MIXED_AGGS, n_keys=1, n_value_cols=2,
                                   val_is_f64=(0,), **SMALL)


@pytest.mark.gpu
def test_mixed_config_dtypes_and_device_equals_host():
    """An f64 and an i64 column in one operator: each aggregate follows its
    own column's flag, is_f64 marks SUM / MAX_RETRACT / MEDIAN of the f64
    column (and AVG), and the device surface emits what the host surface
    emits (exact-class values: bit for bit)."""
    key, a, b, retr = mixed_stream(17)
    script = batches_of(key, [a, b], retr, [700, 700, len(key) - 1400])
    eh, sh, gh = run_script(mixed_cfg, script, device=False, exact_sums=True)
    ed, sd, gd = run_script(mixed_cfg, script, device=True, exact_sums=True)
    assert [str(d) for d in gh.dtypes] == [
        "int64", "float64", "int64", "int64", "float64", "float64",
        "float64", "int64", "int64", "int64"]
    assert gd.dtypes == gh.dtypes
    assert [sorted(r) for r in ed] == [sorted(r) for r in eh]
    assert sd == sh


@pytest.mark.gpu
def test_checkpoint_roundtrip_mid_stream():
    """drain -> restore into a fresh operator of the same config, mid
    stream, continues to the state of the uninterrupted run (state words
    travel raw, f64 sums and float-encoded chains included)."""
    key, a, b, retr = mixed_stream(18)
    mid = len(key) // 2
    cols = lambda sl: [key[sl], a[sl], b[sl], retr[sl]]
    first, second = slice(0, mid), slice(mid, len(key))
    _, want, _ = run_script(
        mixed_cfg, [("batch", cols(first)), ("flush",),
                    ("batch", cols(second)), ("flush",)], exact_sums=True)
    g1 = Gpu(mixed_cfg())
    g1.process(cols(first))
    state = fold({}, g1.flush())
    d0, d1 = g1.op.checkpoint_drain(0), g1.op.checkpoint_drain(1)
    g1.close()
    assert len(d0[0]) > 0 and len(d1[0]) > 0
    g2 = Gpu(mixed_cfg())
    g2.op.restore(0, d0)
    g2.op.restore(1, d1)
    g2.process(cols(second))
    fold(state, g2.flush())
    g2.close()
    assert state == want


@pytest.mark.gpu
def test_create_time_rejections():
    from arroyo_amd import gpu

    def rejected(cfg, pattern):
        with pytest.raises(RuntimeError, match=pattern):
            gpu.make_updagg_op(cfg).close()

    for op in (C.BIT_AND, C.BIT_OR, C.BIT_XOR):
        rejected(cabi.make_updagg_config([(op, 1)], n_value_cols=2,
                                         val_is_f64=(1,), **SMALL),
                 f"bitwise aggregate op {op} over f64 value column 1")
    # the same aggregate over the unflagged column is fine
    gpu.make_updagg_op(cabi.make_updagg_config(
        [(C.BIT_XOR, 0)], n_value_cols=2, val_is_f64=(1,), **SMALL)).close()
    rejected(cabi.make_updagg_config([(C.SUM, 0)], n_value_cols=2,
                                     val_is_f64=(2,), **SMALL),
             r"val_is_f64\[2\] set, but there are 2 value columns")
    cfg = cabi.make_updagg_config([(C.SUM, 0)], n_value_cols=2, **SMALL)
    cfg.val_is_f64[1] = 2
    rejected(cfg, r"val_is_f64\[1\] = 2 \(0 or 1\)")


@pytest.mark.gpu
def test_zeroed_flags_are_the_i64_operator():
    """All-zero val_is_f64 is the operator as it was: the emitted rows of
    an i64 stream equal the C oracle's, bit for bit, aggregate by
    aggregate (the oracle does not read the field)."""
    import oracle
    from arroyo_amd import gpu
    rng = np.random.default_rng(19)
    key, (v,), retr = exact_stream(rng, 3000, 8, 1, 1000)
    v = i64(v)
    # the oracle has no order statistics: those have their own model
    aggs = [(C.COUNT, -1), (C.SUM, 0), (C.AVG, 0), (C.COUNT_DISTINCT, 0),
            (C.BIT_XOR, 0), (C.BIT_AND, 0), (C.BIT_OR, 0), (C.COUNT, 0)]
    cfg = cabi.make_updagg_config(aggs, n_keys=1, n_value_cols=1,
                                  val_is_f64=())
    assert not any(cfg.val_is_f64)
    g, o = gpu.make_updagg_op(cfg), oracle.make_updagg_op(cfg)
    try:
        for lo in range(0, len(key), 1000):
            sl = slice(lo, lo + 1000)
            for op in (g, o):
                op.process_batch([key[sl], v[sl], retr[sl]])
            got, want = g.flush(), o.flush()
            assert [c.dtype for c in got] == [c.dtype for c in want]
            rows = lambda cols: sorted(
                tuple(int(c.view(np.int64)[r]) for c in cols)
                for r in range(len(cols[0])))
            assert rows(got) == rows(want)
    finally:
        g.close()
        o.close()
