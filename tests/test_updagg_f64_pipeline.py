"""The raw debezium fixture through map -> updating aggregate over the device
surfaces, with Float64 columns end to end:

    SELECT product, sum(price * quantity), avg(price), min(price),
           max(price), median(price), count(*) FROM orders GROUP BY product

The map computes price * I2F(quantity) and passes is_retract through; its
device output columns go into updagg_process_batch_device as the addresses
they came back as.  The emitted debezium stream is merged as
tests/test_updagg.py merges it and the final state compared with the Python
model (tests/updagg_f64_ref.py): counts and order statistics exactly, the
sums within the model's bound.  MIN / MAX of the product column pin the
per-row products bit for bit, as does the map's host surface over every
row."""
import numpy as np
import pytest

from arroyo_amd import cabi
from arroyo_amd.cabi import MOP_FMUL, MOP_I2F
from tests import updagg_f64_ref as ref
from tests.test_updagg_f64 import (check_state, event_rows, fold, i64,
                                   load_events, plane_np)

C = cabi


@pytest.mark.gpu
def test_debezium_prices_through_map_and_updagg():
    import torch
    from arroyo_amd import gpu
    events = load_events()
    assert len(events) == 830
    assert sorted({e["op"] for e in events}) == ["c", "d", "u"]
    names = sorted({r["product_name"] for r, _ in event_rows(events)})

    # [product, quantity, price, is_retract] -> [product, price * quantity,
    # price, is_retract]
    mp = gpu.make_map_op(cabi.make_map_config(
        n_in_cols=4, prog=[(MOP_I2F, 1, 0, 4), (MOP_FMUL, 4, 2, 5)],
        out_reg=[0, 5, 2, 3], out_is_f64=[0, 1, 1, 0]))
    aggs = [(C.SUM, 0), (C.AVG, 1), (C.MIN_RETRACT, 1), (C.MAX_RETRACT, 1),
            (C.MEDIAN, 1), (C.COUNT, -1), (C.MIN_RETRACT, 0),
            (C.MAX_RETRACT, 0)]
    cfg = lambda: cabi.make_updagg_config(
        aggs, n_keys=1, n_value_cols=2, val_is_f64=(0, 1),
        log2_capacity=10, log2_nodes=14, log2_out_cap=12)
    agg = gpu.make_updagg_op(cfg())
    model = ref.RefF64UpdAgg(cfg())
    dev = torch.device("cuda", 0)

    state, all_cols = {}, []
    try:
        for lo in range(0, len(events), 120):      # a flush every ~120 events
            rows = event_rows(events[lo:lo + 120])
            prod = i64([names.index(r["product_name"]) for r, _ in rows])
            qty = i64([r["quantity"] for r, _ in rows])
            price = np.array([float(r["price"]) for r, _ in rows])
            retr = i64([d for _, d in rows])
            cols = [prod, qty, plane_np(price), retr]
            all_cols.append(cols)
            t = [torch.from_numpy(c.copy()).to(dev) for c in cols]
            torch.cuda.synchronize()
            outp, n_out = mp.process_batch_device([x.data_ptr() for x in t],
                                                  len(prod))
            assert n_out == len(prod)
            agg.process_batch_device(outp, n_out)
            out = agg.flush()
            assert [str(c.dtype) for c in out] == \
                ["int64"] + ["float64"] * 5 + ["int64", "float64", "float64",
                                               "int64"]
            words = [c.view(np.int64) for c in out]
            fold(state, [(int(words[0][r]),)
                         + tuple((int(w[r]), True) for w in words[1:-1])
                         + (int(words[-1][r]),)
                         for r in range(len(words[0]))])
            model.process_batch([prod, plane_np(price * qty), plane_np(price),
                                 retr])
            check_state(state, model.flush(), what=f"events {lo}..")

        # every row's product, bit for bit, through the map's host surface
        whole = [np.concatenate([b[c] for b in all_cols]) for c in range(4)]
        got = mp.process_batch(whole)
        assert got[1].dtype == np.float64
        want = whole[2].view(np.float64) * whole[1]
        assert np.array_equal(got[1].view(np.int64), want.view(np.int64))
    finally:
        mp.close()
        agg.close()

    assert len(state) == 6
    for k in state:
        assert 85 <= state[k][5][0] <= 104
