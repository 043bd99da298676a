"""Window functions beyond ROW_NUMBER (ranks, LAG/LEAD, framed aggregates)
against tests/windowfn_ref.py, an independent restatement of the rules in
include/arroyo_amd_types.h (restated from DataFusion 48, not golden-pinned).
Every comparison is bit-exact; with limit == 0 the output row order is
pinned too (instants by timestamp, then partition, ORDER BY, arrival)."""
import ctypes

import numpy as np
import pytest

import oracle
from arroyo_amd import cabi
from tests import windowfn_ref as ref

NS = 10**9
T0 = 1_600_000_000 * NS
U64MAX = 2**64 - 1
I64MIN, I64MAX = -2**63, 2**63 - 1
T = cabi.WFN_SCAN_TILE

FN = {"row_number": cabi.WFN_ROW_NUMBER, "rank": cabi.WFN_RANK,
      "dense_rank": cabi.WFN_DENSE_RANK, "lag": cabi.WFN_LAG,
      "lead": cabi.WFN_LEAD, "first_value": cabi.WFN_FIRST_VALUE,
      "last_value": cabi.WFN_LAST_VALUE, "sum": cabi.WFN_SUM,
      "count": cabi.WFN_COUNT, "min": cabi.WFN_MIN, "max": cabi.WFN_MAX}
FRAME = {"range": cabi.WFN_FRAME_RANGE, "rows": cabi.WFN_FRAME_ROWS,
         "partition": cabi.WFN_FRAME_PARTITION}
# every function with every frame it may be given
LEGAL = [(f, "range") for f in ("rank", "dense_rank", "lag", "lead")] + \
        [(f, fr) for f in ref.FRAMED for fr in ref.FRAMES]


def i64(x):
    return np.ascontiguousarray(x, dtype=np.int64)


# ------------------------------------------------------------ the reference


def test_reference_reproduces_the_worked_example():
    part = [1, 1, 1, 1, 2, 2]
    o = [5, 7, 5, 7, 3, 3]
    arg = [10, 20, 30, 40, 50, 60]
    lay = ref.Layout(part, [(o, True)])

    def by_row(fn, **kw):
        vals = lay.values(arg, fn, **kw)
        out = [None] * 6
        for pos, (v, ok) in enumerate(vals):
            out[lay.rows[pos]] = v if ok else None
        return out

    assert by_row("row_number") == [3, 1, 4, 2, 1, 2]
    assert by_row("rank") == [3, 1, 3, 1, 1, 1]
    assert by_row("dense_rank") == [2, 1, 2, 1, 1, 1]
    assert by_row("lag", k=1) == [40, None, 10, 20, None, 50]
    assert by_row("lead", k=1) == [30, 40, None, 10, 60, None]
    assert by_row("sum", frame="rows") == [70, 20, 100, 60, 50, 110]
    assert by_row("sum", frame="range") == [100, 60, 100, 60, 110, 110]
    assert by_row("max", frame="rows") == [40, 20, 40, 40, 50, 60]
    assert by_row("last_value", frame="range") == [30, 40, 30, 40, 60, 60]
    assert by_row("last_value", frame="partition") == \
        [30, 30, 30, 30, 60, 60]
    # beyond the table: defaults, k = 0, wrapping, count
    assert by_row("lag", k=1, default=-7) == [40, -7, 10, 20, -7, 50]
    assert by_row("lag", k=0) == arg
    assert by_row("count", frame="range") == [4, 2, 4, 2, 2, 2]
    assert by_row("first_value") == [20, 20, 20, 20, 50, 50]
    assert ref.wrap64(I64MAX + 1) == I64MIN
    lay1 = ref.Layout(None, [([0, 0], False)])
    assert lay1.values([I64MAX, 1], "sum", frame="rows") == \
        [(I64MAX, True), (I64MIN, True)]


# ------------------------------------------------- create-time validation


def _create(cfg):
    from arroyo_amd import gpu
    return gpu.make_windowfn_op(cfg)


def _rejected(match, **kw):
    base = dict(n_cols=4, part_col=0, order=[(1, True)])
    base.update(kw)
    with pytest.raises(RuntimeError, match=match) as e:
        _create(cabi.make_windowfn_config(**base))
    assert "hipSetDevice" not in str(e.value), \
        "rejected before a device is looked for"


def _accepted(cfg):
    """A valid config gets past validation: the create works, or fails
    only for want of a device."""
    try:
        op = _create(cfg)
    except RuntimeError as e:
        assert "hipSetDevice" in str(e), str(e)
    else:
        op.close()


def test_create_rejects_unknown_function_and_frame():
    _rejected("unknown window function 11", fn=11)
    _rejected("unknown window function -1", fn=-1)
    _rejected("unknown window frame 3", fn=cabi.WFN_SUM, arg_col=2, frame=3)
    _rejected("unknown window frame -1", fn=cabi.WFN_SUM, arg_col=2,
              frame=-1)


@pytest.mark.parametrize("name", ref.TAKES_ARG)
def test_create_rejects_arg_col_out_of_range(name):
    # n_cols = 4: data columns 0..2, column 3 is the timestamp
    for bad in (-1, 3, 4, -2):
        _rejected(r"arg_col -?\d+ out of range \[0, 2\]", fn=FN[name],
                  arg_col=bad)
    _accepted(cabi.make_windowfn_config(4, 0, [(1, True)], fn=FN[name],
                                        arg_col=2))


def test_create_rejects_arg_col_where_none_is_taken():
    for name in ("rank", "dense_rank"):
        _rejected("arg_col must be -1", fn=FN[name], arg_col=0)
        _accepted(cabi.make_windowfn_config(4, 0, [(1, True)], fn=FN[name]))
    _rejected("arg_col must be -1", fn=cabi.WFN_ROW_NUMBER, arg_col=1)
    # COUNT takes a column or none
    _rejected(r"arg_col 3 out of range", fn=cabi.WFN_COUNT, arg_col=3)
    _accepted(cabi.make_windowfn_config(4, 0, [(1, True)], fn=cabi.WFN_COUNT))
    _accepted(cabi.make_windowfn_config(4, 0, [(1, True)], fn=cabi.WFN_COUNT,
                                        arg_col=2))


def test_create_rejects_negative_offset():
    _rejected("offset must be >= 0, got -1", fn=cabi.WFN_LAG, arg_col=2,
              offset=-1)
    _accepted(cabi.make_windowfn_config(4, 0, [(1, True)], fn=cabi.WFN_LAG,
                                        arg_col=2, offset=0))


def test_create_rejects_limit_outside_the_rank_family():
    for name in ref.FUNCTIONS[3:]:
        _rejected("limit is only for ROW_NUMBER, RANK and DENSE_RANK",
                  fn=FN[name], arg_col=2, limit=3)
    for name in ("rank", "dense_rank"):
        _accepted(cabi.make_windowfn_config(4, 0, [(1, True)], fn=FN[name],
                                            limit=3))


def test_create_rejects_a_frame_where_frames_are_ignored():
    for name in ("row_number", "rank", "dense_rank"):
        for frame in (1, 2):
            _rejected("frame must be 0", fn=FN[name], frame=frame)
    for name in ("lag", "lead"):
        _rejected("frame must be 0", fn=FN[name], arg_col=2, frame=1)
    for name, frame in LEGAL:
        _accepted(cabi.make_windowfn_config(
            4, 0, [(1, True)], fn=FN[name], frame=FRAME[frame],
            arg_col=2 if name in ref.TAKES_ARG else -1))


def test_zeroed_tail_is_row_number():
    """A caller that fills only the fields from before the functions."""
    cfg = cabi.AmdWindowFnConfig()
    cfg.n_cols, cfg.part_col, cfg.n_order = 3, 0, 1
    cfg.order_col[0], cfg.order_desc[0] = 1, 1
    assert (cfg.fn, cfg.arg_col, cfg.frame, cfg.offset, cfg.has_default) == \
        (cabi.WFN_ROW_NUMBER, 0, cabi.WFN_FRAME_RANGE, 0, 0)
    _accepted(cfg)
    made = cabi.make_windowfn_config(3, 0, [(1, True)])
    assert (made.fn, made.arg_col, made.frame, made.offset) == (0, -1, 0, 1)


def test_oracle_refuses_everything_but_row_number():
    for name in ref.FUNCTIONS[1:]:
        with pytest.raises(ValueError, match="oracle implements ROW_NUMBER "
                                             "only"):
            oracle.make_windowfn_op(cabi.make_windowfn_config(
                4, 0, [(1, True)], fn=FN[name],
                arg_col=2 if name in ref.TAKES_ARG else -1))
    oracle.make_windowfn_op(
        cabi.make_windowfn_config(4, 0, [(1, True)])).close()


# ------------------------------------------------------------- GPU helpers


def raw_watermark(op, wm):
    """handle_watermark through the raw ABI: (columns, bitmap bytes per
    column or None, whether the batch carries a validity table)."""
    out = cabi.AmdOutBatch()
    op._call("handle_watermark", wm, ctypes.byref(out))
    cols = cabi._out_to_numpy(out)
    n = out.n_rows
    has_table = bool(out.validity)
    bms = []
    for c in range(out.n_cols):
        if not has_table or not out.validity[c]:
            bms.append(None)
            continue
        bms.append(bytes(ctypes.cast(out.validity[c], ctypes.POINTER(
            ctypes.c_uint8 * ((n + 7) // 8))).contents))
    op._fn["free_out"](ctypes.byref(out))
    return cols, bms, has_table


def gpu_run(cols, part_col, order, name, steps=None, arg_col=-1,
            frame="range", k=1, default=None, limit=0, log2_rows_cap=12,
            instants=64, log2_out_cap=16):
    """Feed `cols` (arrival order) and fire; steps = [(row slice, watermark
    or None)], default: everything, then one final watermark.  Returns the
    output rows in output order and the function column's validity."""
    from arroyo_amd import gpu
    op = gpu.make_windowfn_op(cabi.make_windowfn_config(
        n_cols=len(cols), part_col=part_col, order=order, limit=limit,
        log2_rows_cap=log2_rows_cap, instants=instants,
        log2_out_cap=log2_out_cap, fn=FN[name], arg_col=arg_col,
        frame=FRAME[frame], offset=k, default=default))
    rows, valid = [], []
    for sl, wm in steps or [(slice(None), U64MAX)]:
        if sl is not None and len(cols[0][sl]):
            op.process_batch([i64(c[sl]) for c in cols])
        if wm is None:
            continue
        out, masks = op.handle_watermark_with_validity(wm)
        assert len(out) == len(cols) + 1
        rows += list(zip(*(c.tolist() for c in out)))
        valid += masks[-1].tolist()
        assert all(m.all() for m in masks[:-1])
    op.close()
    return rows, valid


def check(cols, part_col, order, name, steps=None, **kw):
    """GPU against the reference: values, validity and, without a limit,
    the row order."""
    gkw = {k: kw.pop(k) for k in ("log2_rows_cap", "instants",
                                  "log2_out_cap") if k in kw}
    got, gvalid = gpu_run(cols, part_col, order, name, steps, **kw, **gkw)
    want, wvalid = ref.window_rows(cols, part_col, order, name, **kw)
    if kw.get("limit"):
        assert all(gvalid) and all(wvalid)
        got, want = sorted(got), sorted(want)
    assert len(got) == len(want)
    assert got == want
    assert gvalid == wvalid
    return want, wvalid


# ---------------------------------------------------------------- edge grid


def grid_sizes():
    """Partitions laid back to back so that their boundaries fall on, just
    before and just after the seams of a wave (64 rows), a block's pass
    (256) and a scan tile (T); every size is from the issue's set."""
    assert T % 256 == 0 and T >= 1536
    sizes = [63, 65, 65, 63, 255, 1, 1, 255, 257, 255]
    sizes += [256] * ((T - 256 - sum(sizes)) // 256)
    sizes += [255, 1, 1, T - 1, T, T + 1, 2 * T + 1, 64, 256, 2]
    allowed = {1, 2, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 2 * T + 1}
    assert set(sizes) == allowed
    return sizes


@pytest.fixture(scope="module")
def grid():
    sizes = grid_sizes()
    bounds = np.cumsum(sizes)
    for seam in (64, 256, T):
        assert {0, 1, seam - 1} <= {int(b) % seam for b in bounds}, seam
    rng = np.random.default_rng(5)
    n = int(bounds[-1])
    part = np.repeat(np.arange(len(sizes)), sizes).astype(np.int64) * 3 - 7
    o = rng.integers(0, 3, size=n).astype(np.int64)
    single = sizes.index(64)          # one partition that is one peer group
    o[part == single * 3 - 7] = 1
    arg = rng.choice(np.array([I64MIN, I64MAX, -1, 0, 1, 12345, -99999],
                              dtype=np.int64), size=n)
    assert {I64MIN, I64MAX, -1, 0} <= set(arg.tolist())
    ts = np.full(n, T0, dtype=np.int64)
    # arrival order is not sort order
    sh = rng.permutation(n)
    cols = [part[sh], o[sh], arg[sh], ts]
    lay = ref.Layout(cols[0], [(cols[1], True)])
    groups = lay.peer_groups()
    assert max(b - a + 1 for a, b in groups) >= 3
    assert any(a < s <= b for a, b in groups for s in range(T, n, T)), \
        "a peer group straddles a tile seam"
    assert any((a, b) in set(lay.partitions()) and b - a + 1 == 64
               for a, b in groups), "a partition of one peer group"
    # SUM really wraps somewhere
    raw = [0]
    for pos in range(n):
        raw.append((0 if pos == lay.p0[pos] else raw[-1])
                   + int(cols[2][lay.rows[pos]]))
    assert any(not I64MIN <= s <= I64MAX for s in raw)
    return cols


@pytest.mark.gpu
@pytest.mark.parametrize("name,frame", LEGAL)
def test_edge_grid(grid, name, frame):
    check(grid, 0, [(1, True)], name, frame=frame,
          arg_col=2 if name in ref.TAKES_ARG else -1, log2_rows_cap=14,
          instants=2)


VARIANT_FNS = [("rank", "range"), ("dense_rank", "range"), ("lag", "range"),
               ("lead", "range"), ("sum", "rows"), ("last_value", "range"),
               ("max", "range"), ("min", "partition"), ("count", "range"),
               ("first_value", "rows")]


def small_stream(seed, n=3000, n_instants=1, parts=5):
    rng = np.random.default_rng(seed)
    part = rng.integers(0, parts, size=n).astype(np.int64)
    o1 = rng.integers(0, 4, size=n).astype(np.int64)
    o2 = rng.integers(-2, 2, size=n).astype(np.int64)
    arg = rng.choice(np.array([I64MIN, I64MAX, -1, 0, 7, -123456789],
                              dtype=np.int64), size=n)
    ts = np.sort(T0 + rng.integers(0, n_instants, size=n) * NS)
    return [part, o1, o2, arg, ts.astype(np.int64)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,frame", VARIANT_FNS)
def test_whole_instant_partition(name, frame):
    check(small_stream(21), -1, [(1, False)], name, frame=frame,
          arg_col=3 if name in ref.TAKES_ARG else -1)


@pytest.mark.gpu
@pytest.mark.parametrize("name,frame", VARIANT_FNS)
def test_two_order_columns_mixed_direction(name, frame):
    check(small_stream(22), 0, [(1, True), (2, False)], name, frame=frame,
          arg_col=3 if name in ref.TAKES_ARG else -1)


@pytest.mark.gpu
@pytest.mark.parametrize("name,frame", VARIANT_FNS)
def test_arrival_order_over_two_batches_decides_peer_order(name, frame):
    cols = small_stream(23)
    n = len(cols[0])
    # the second batch's rows tie with the first's on (part, o1)
    steps = [(slice(0, n // 3), None), (slice(n // 3, n), U64MAX)]
    check(cols, 0, [(1, True)], name, steps, frame=frame,
          arg_col=3 if name in ref.TAKES_ARG else -1)


# ----------------------------------------------------------------- LAG/LEAD

LL_M = 100   # the partition whose size the distances are about


def lag_stream():
    rng = np.random.default_rng(31)
    sizes = [LL_M, 7, 1, 70]
    part = np.repeat(np.arange(len(sizes)), sizes).astype(np.int64)
    n = len(part)
    o = rng.integers(0, 5, size=n).astype(np.int64)
    arg = rng.integers(-1000, 1000, size=n).astype(np.int64)
    arg[:4] = [I64MIN, I64MAX, -1, 0]
    sh = rng.permutation(n)
    return [part[sh], o[sh], arg[sh], np.full(n, T0, dtype=np.int64)]


def check_bitmap(cols, name, k, default, steps_in=None):
    """One handle_watermark through the raw ABI: values, NULL positions
    and the bitmap's bytes, padding included."""
    from arroyo_amd import gpu
    op = gpu.make_windowfn_op(cabi.make_windowfn_config(
        n_cols=len(cols), part_col=0, order=[(1, False)], log2_rows_cap=10,
        instants=16, log2_out_cap=12, fn=FN[name], arg_col=2, offset=k,
        default=default))
    op.process_batch(cols)
    out, bms, has_table = raw_watermark(op, U64MAX)
    op.close()
    want, wvalid = ref.window_rows(cols, 0, [(1, False)], name, arg_col=2,
                                   k=k, default=default)
    assert list(zip(*(c.tolist() for c in out))) == want
    assert all(b is None for b in bms[:-1])
    if all(wvalid):
        assert not has_table and bms[-1] is None
    else:
        assert has_table
        assert bms[-1] == np.packbits(np.array(wvalid),
                                      bitorder="little").tobytes()
    return wvalid


@pytest.mark.gpu
@pytest.mark.parametrize("k", [0, 1, 2, 64, LL_M, LL_M + 1])
@pytest.mark.parametrize("name", ["lag", "lead"])
def test_lag_lead_distances(name, k):
    cols = lag_stream()
    wvalid = check_bitmap(cols, name, k, None)
    # NULLs exactly where the distance leaves the partition
    assert all(wvalid) == (k == 0)
    if k >= LL_M:
        assert not any(wvalid)
    assert all(check_bitmap(cols, name, k, -7))
    assert all(check_bitmap(cols, name, k, I64MIN))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["lag", "lead"])
def test_lag_lead_bitmap_across_instants(name):
    """Several instants fire in one handle_watermark with row counts that
    are no multiple of 8: each instant's bits are appended at a bit offset."""
    rng = np.random.default_rng(32)
    counts = [13, 70, 1, 129, 67, 3]
    assert all(c % 8 for c in counts)
    ts = np.repeat(T0 + np.arange(len(counts)) * NS, counts).astype(np.int64)
    n = len(ts)
    sh = rng.permutation(n)
    cols = [rng.integers(0, 3, size=n).astype(np.int64),
            rng.integers(0, 4, size=n).astype(np.int64),
            rng.integers(-50, 50, size=n).astype(np.int64), ts[sh]]
    wvalid = check_bitmap(cols, name, 1, None)
    assert 0 < sum(wvalid) < n


# -------------------------------------------------------------------- limit


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["rank", "dense_rank"])
def test_limit_keeps_ties(name):
    rng = np.random.default_rng(41)
    n = 3000
    cols = [rng.integers(0, 6, size=n).astype(np.int64),
            rng.integers(0, 5, size=n).astype(np.int64),   # heavy ties
            np.sort(T0 + rng.integers(0, 4, size=n) * NS).astype(np.int64)]
    assert len(np.unique(cols[2])) >= 3
    want, _ = check(cols, 0, [(1, True)], name, limit=3)
    assert all(r[-1] <= 3 for r in want)
    kept = {}
    for r in want:
        kept[(r[2], r[0])] = kept.get((r[2], r[0]), 0) + 1
    assert max(kept.values()) > 3, "ties past 3 are kept"
    if name == "rank":
        # RANK skips: a tie for first place can leave no rank 2
        assert {r[-1] for r in want} <= {1, 2, 3}


# --------------------------------------------------------------- carry seam

SEAM_N = 257 * T + 1


@pytest.fixture(scope="module")
def seam():
    """One instant of 257 * T + 1 rows, as one partition and as 1000: the
    sort and the expected SUM/ROWS and MAX/RANGE, vectorised."""
    rng = np.random.default_rng(51)
    o = rng.integers(0, 200, size=SEAM_N).astype(np.int64)
    arg = rng.integers(I64MIN, I64MAX, size=SEAM_N, dtype=np.int64,
                       endpoint=True)
    ts = np.full(SEAM_N, T0, dtype=np.int64)
    made = {}
    for n_parts in (1, 1000):
        part = rng.integers(0, n_parts, size=SEAM_N).astype(np.int64)
        perm = np.lexsort((np.arange(SEAM_N), o, part))
        sp, so, sa = part[perm], o[perm], arg[perm]
        head = np.r_[True, sp[1:] != sp[:-1]]
        starts = np.flatnonzero(head)
        ends = np.r_[starts[1:], SEAM_N]
        sums, maxs = np.empty_like(sa), np.empty_like(sa)
        with np.errstate(over="ignore"):
            for a, b in zip(starts, ends):
                sums[a:b] = np.add.accumulate(sa[a:b])      # wraps
                maxs[a:b] = np.maximum.accumulate(sa[a:b])
        change = head[1:] | (so[1:] != so[:-1])
        gid = np.cumsum(np.r_[0, change])
        pe = np.flatnonzero(np.r_[change, True])[gid]       # peer-group end
        made[n_parts] = ([part, o, arg, ts], perm,
                         {"sum": sums, "max": maxs[pe]})
    return made


@pytest.mark.gpu
@pytest.mark.parametrize("name,frame", [("sum", "rows"), ("max", "range")])
@pytest.mark.parametrize("n_parts", [1, 1000])
def test_carry_seam(seam, n_parts, name, frame):
    """The smallest shape whose tile partials reach the second 256-chunk of
    the partial scan, whose carry then crosses (or, with 1000 partitions,
    must not cross) the chunk seam."""
    from arroyo_amd import gpu
    cols, perm, want = seam[n_parts]
    assert -(-SEAM_N // T) > 256
    op = gpu.make_windowfn_op(cabi.make_windowfn_config(
        n_cols=4, part_col=0, order=[(1, False)], log2_rows_cap=20,
        instants=2, log2_out_cap=20, fn=FN[name], arg_col=2,
        frame=FRAME[frame]))
    op.process_batch(cols)
    out, masks = op.handle_watermark_with_validity(U64MAX)
    op.close()
    for c in range(4):
        assert np.array_equal(out[c], cols[c][perm]), c
    assert np.array_equal(out[4], want[name])
    assert masks[4].all()


# --------------------------------------------------------------------- fuzz


def fuzz_case(seed):
    rng = np.random.default_rng(1000 + seed)
    name, frame = LEGAL[int(rng.integers(0, len(LEGAL)))]
    if seed < len(ref.FUNCTIONS) - 1:
        name = ref.FUNCTIONS[1 + seed]          # every function at least once
        frame = ref.FRAMES[seed % 3] if name in ref.FRAMED else "range"
    order = [(1, bool(rng.integers(0, 2)))]
    if rng.integers(0, 2):
        order.append((2, bool(rng.integers(0, 2))))
    kw = dict(frame=frame, arg_col=3 if name in ref.TAKES_ARG else -1)
    if name in ("lag", "lead"):
        kw["k"] = int(rng.choice([0, 1, 2, 3, 17, 500]))
        kw["default"] = None if rng.integers(0, 2) else int(rng.integers(-9, 9))
    if name in ("rank", "dense_rank") and rng.integers(0, 2):
        kw["limit"] = 3
    n_instants = int(rng.integers(1, 31))
    return name, order, kw, n_instants


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(20))
def test_fuzz(seed):
    name, order, kw, n_instants = fuzz_case(seed)
    cols = small_stream(2000 + seed, n=4000, n_instants=n_instants, parts=6)
    ts = cols[-1]
    mid = int(T0 + (n_instants // 2) * NS)
    first = int(np.searchsorted(ts, mid))       # rows with ts < mid
    steps = [(slice(0, first), mid), (slice(first, None), U64MAX)]
    part_col = -1 if seed % 5 == 4 else 0
    check(cols, part_col, order, name, steps, **kw)


# ------------------------------------------------ checkpoint, device ingest


@pytest.mark.gpu
@pytest.mark.parametrize("name,frame", [("lag", "range"), ("sum", "rows")])
def test_checkpoint_roundtrip(name, frame):
    """Ties make both depend on arrival order (LAG takes no frame; SUM
    runs under ROWS): drain at half the stream, restore into a fresh
    handle, finish, and match the uninterrupted run and the reference."""
    from arroyo_amd import gpu
    cols = small_stream(61, n=3000, n_instants=12)
    n = len(cols[0])
    kw = dict(n_cols=5, part_col=0, order=[(1, False)], log2_rows_cap=12,
              instants=64, fn=FN[name], arg_col=3, frame=FRAME[frame])
    a = gpu.make_windowfn_op(cabi.make_windowfn_config(**kw))
    a.process_batch([c[:n // 2] for c in cols])
    drained = a.checkpoint_drain()
    a.close()
    assert len(drained[0]) == n // 2
    b = gpu.make_windowfn_op(cabi.make_windowfn_config(**kw))
    b.restore(drained)
    b.process_batch([c[n // 2:] for c in cols])
    got, gmask = b.handle_watermark_with_validity(U64MAX)
    b.close()
    c_ = gpu.make_windowfn_op(cabi.make_windowfn_config(**kw))
    c_.process_batch(cols)
    straight, smask = c_.handle_watermark_with_validity(U64MAX)
    c_.close()
    for x, y in zip(got, straight):
        assert np.array_equal(x, y)
    assert np.array_equal(gmask[-1], smask[-1])
    want, wvalid = ref.window_rows(cols, 0, [(1, False)], name, arg_col=3,
                                   frame=frame)
    assert list(zip(*(c.tolist() for c in got))) == want
    assert gmask[-1].tolist() == wvalid


@pytest.mark.gpu
def test_device_resident_ingest_matches_host():
    import torch
    from arroyo_amd import gpu
    cols = small_stream(62, n=3000, n_instants=9)
    kw = dict(n_cols=5, part_col=0, order=[(1, True)], log2_rows_cap=12,
              instants=64, fn=cabi.WFN_SUM, arg_col=3,
              frame=cabi.WFN_FRAME_RANGE)
    h = gpu.make_windowfn_op(cabi.make_windowfn_config(**kw))
    d = gpu.make_windowfn_op(cabi.make_windowfn_config(**kw))
    h.process_batch(cols)
    dev = torch.device("cuda", 0)
    tens = [torch.from_numpy(c.copy()).to(dev) for c in cols]
    torch.cuda.synchronize()
    d.process_batch_device([t.data_ptr() for t in tens], len(cols[0]))
    got = d.handle_watermark(U64MAX)
    want = h.handle_watermark(U64MAX)
    h.close()
    d.close()
    assert len(want[0]) == len(cols[0])
    for x, y in zip(got, want):
        assert np.array_equal(x, y)
    rows, _ = ref.window_rows(cols, 0, [(1, True)], "sum", arg_col=3)
    assert list(zip(*(c.tolist() for c in got))) == rows
