"""SQL NULLs end to end on the GPU: LEFT instant join -> nullable map ->
updating aggregate with null_semantics = 1.  Every stage uses its nullable
surface, and the Arrow bitmaps one stage returns are handed to the next as
the pointers they came back as -- nothing decodes or rebuilds them on the
way.

The map runs the anti-join

    SELECT l.k, l.v + COALESCE(r.v, 0), r.v FROM l LEFT JOIN r ...
    WHERE r.v IS NULL

and the aggregate groups what survives.  Expected values are computed in
numpy from the inputs.  A second test runs session_window.sql's
CASE WHEN counter % 10 = 0 THEN 0 ELSE counter END as a SELECT program."""
import ctypes

import numpy as np
import pytest

from arroyo_amd import cabi
from arroyo_amd.cabi import (MOP_ADD, MOP_COALESCE, MOP_CONST, MOP_EQ,
                             MOP_IS_NULL, MOP_MOD, MOP_SELECT)

T0 = 1_600_000_000 * 10**9
_VPP = ctypes.POINTER(ctypes.c_void_p)


def _validity_ptr(out):
    """out->validity as the next stage's validity argument, untouched."""
    return ctypes.cast(out.validity, _VPP)


@pytest.mark.gpu
def test_left_join_anti_join_map_into_nullable_aggregate():
    from arroyo_amd import gpu
    rng = np.random.default_rng(21)
    n_left, n_keys = 300, 37
    lk = rng.integers(0, n_keys, size=n_left).astype(np.int64)
    lv = rng.integers(-1000, 1000, size=n_left).astype(np.int64)
    # the right side matches every third key; 0 is a value, not a NULL
    rk = np.arange(0, n_keys, 3, dtype=np.int64)
    rv = (rk * 10).astype(np.int64)
    assert rv[0] == 0

    join = gpu.make_join_op(cabi.make_join_config(
        n_keys=1, n_left_vals=1, n_right_vals=1, join_type=cabi.JOIN_LEFT))
    join.process_batch(join.LEFT, [lk, lv, np.full(n_left, T0)])
    join.process_batch(join.RIGHT, [rk, rv, np.full(len(rk), T0)])
    j = cabi.AmdOutBatch()
    join._call("handle_watermark", T0 + 1, ctypes.byref(j))
    # [key, l.v, r.v, instant, l present, r present]
    assert j.n_cols == 6 and j.n_rows == n_left
    jm = cabi.out_validity(j)
    jc = cabi._out_to_numpy(j)
    matched = np.isin(lk, rk)
    assert jm[2] is not None and (~jm[2]).sum() == (~matched).sum() > 0
    assert np.array_equal(jm[2], jc[5].astype(bool))

    # r6 = r.v IS NULL; r8 = COALESCE(r.v, 0); r9 = l.v + r8; r10 = 0
    prog = [(MOP_IS_NULL, 2, 0, 6), (MOP_CONST, 0, 0, 7, 0),
            (MOP_COALESCE, 2, 7, 8), (MOP_ADD, 1, 8, 9),
            (MOP_CONST, 0, 0, 10, 0)]
    mp = gpu.make_map_op(cabi.make_map_config(
        n_in_cols=6, prog=prog, out_reg=[0, 9, 2, 10], filter_reg=6,
        null_semantics=1))
    m = cabi.AmdOutBatch()
    mp._call("process_batch_nullable", j.cols, _validity_ptr(j), j.n_cols,
             j.n_rows, ctypes.byref(m))
    anti = ~matched
    assert m.n_rows == anti.sum() and m.n_cols == 4
    mm = cabi.out_validity(m)
    mc = cabi._out_to_numpy(m)
    # only r.v carries a bitmap: every kept row has it NULL, value 0
    assert mm[0] is None and mm[1] is None and mm[3] is None
    assert mm[2] is not None and not mm[2].any() and not mc[2].any()
    # the join emits in its own order: compare as (key, value) multisets
    assert sorted(zip(mc[0].tolist(), mc[1].tolist())) == \
        sorted(zip(lk[anti].tolist(), lv[anti].tolist()))

    # [key, l.v + COALESCE(r.v, 0), r.v, is_retract]
    aggs = [(cabi.COUNT, -1), (cabi.SUM, 0), (cabi.SUM, 1), (cabi.COUNT, 1)]
    agg = gpu.make_updagg_op(cabi.make_updagg_config(
        aggs, n_keys=1, n_value_cols=2, null_semantics=True))
    agg._call("process_batch_nullable", m.cols, _validity_ptr(m), m.n_cols,
              m.n_rows)
    cols, masks = agg.flush_with_validity()
    join._fn["free_out"](ctypes.byref(j))
    mp._fn["free_out"](ctypes.byref(m))
    for op in (join, mp, agg):
        op.close()

    # [key, COUNT(*), SUM(l.v + ..), SUM(r.v), COUNT(r.v), is_retract]
    order = np.argsort(cols[0])
    keys = sorted(set(lk[anti].tolist()))
    assert all(k % 3 != 0 for k in keys)
    assert cols[0][order].tolist() == keys
    assert cols[1][order].tolist() == [int((lk[anti] == k).sum())
                                       for k in keys]
    assert cols[2][order].tolist() == [int(lv[anti][lk[anti] == k].sum())
                                       for k in keys]
    assert masks[0].all() and masks[1].all() and masks[2].all()
    assert not masks[3].any() and not cols[3].any()     # SUM(r.v) is NULL
    assert masks[4].all() and not cols[4].any()         # COUNT(r.v) is 0
    assert not cols[5].any()


@pytest.mark.gpu
def test_session_window_case_expression_as_select():
    """user_id = CASE WHEN counter % 10 = 0 THEN 0 ELSE counter END: what
    tests/test_session.py computes with numpy.where on the host."""
    from arroyo_amd import gpu
    counter = np.arange(0, 500, dtype=np.int64)
    prog = [(MOP_CONST, 0, 0, 1, 10), (MOP_MOD, 0, 1, 2),
            (MOP_CONST, 0, 0, 3, 0), (MOP_EQ, 2, 3, 4),
            (MOP_SELECT, 4, 3, 5, 0)]
    op = gpu.make_map_op(cabi.make_map_config(
        n_in_cols=1, prog=prog, out_reg=[5, 0], null_semantics=1))
    cols, masks = op.process_batch_nullable([counter], None)
    op.close()
    user = np.where(counter % 10 == 0, 0, counter).astype(np.int64)
    assert np.array_equal(cols[0], user) and np.array_equal(cols[1], counter)
    assert masks[0].all() and masks[1].all()
