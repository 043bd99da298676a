"""Top-N that keeps ties through the real two-operator pipeline on the GPU:
hop(1min, 1h) COUNT GROUP BY driver_id on the window operator, then
RANK() OVER (PARTITION BY window ORDER BY count DESC) with the downstream
`rank <= 3` filter fused into the window-function operator.  The checker is
tests/windowfn_ref.py applied to the oracle window operator's output for
the same stream."""
import numpy as np
import pytest

import oracle
from arroyo_amd import cabi
from arroyo_amd.pipeline import U64MAX, WatermarkGen, batches_from_columns
from tests import windowfn_ref as ref
from tests.golden_util import NS, load_inputs

HOUR = 3600 * NS


def window_stream(make_window_op, sink):
    """The cars stream through a window operator; sink(rows or None, wm) is
    called once per watermark with the rows it emitted."""
    inp = load_inputs()["cars"]
    ts = np.array(inp["ts"], dtype=np.int64)
    key = np.array(inp["driver_id"], dtype=np.int64)
    win = make_window_op(cabi.make_config(
        width_ns=HOUR, slide_ns=60 * NS, n_keys=1, n_value_cols=0,
        aggs=[(cabi.COUNT, -1)], log2_capacity=14, ring_panes=256))
    wg = WatermarkGen(lateness_ns=HOUR)
    for cols in batches_from_columns([key, ts], 32):
        win.process_batch(cols)
        wm = wg.on_batch(cols[-1])
        if wm is not None:
            out = win.handle_watermark(wm)
            sink(out if out and len(out[0]) else None, wm)
    out = win.handle_watermark(U64MAX)
    sink(out if out and len(out[0]) else None, U64MAX)
    win.close()


@pytest.mark.gpu
def test_rank_top3_with_ties_pipeline_gpu():
    from arroyo_amd import gpu
    # window output columns: [driver, count, ws, we, _ts]
    wf = gpu.make_windowfn_op(cabi.make_windowfn_config(
        n_cols=5, part_col=2, order=[(1, True)], limit=3, log2_rows_cap=12,
        instants=256, fn=cabi.WFN_RANK))
    got = []

    def gpu_sink(out, wm):
        if out is not None:
            wf.process_batch(out)
        res = wf.handle_watermark(wm)
        got.extend(zip(*(c.tolist() for c in res)))

    window_stream(gpu.make_op, gpu_sink)
    wf.close()

    emitted = []
    window_stream(oracle.make_op,
                  lambda out, wm: out is not None and emitted.append(out))
    cols = [np.concatenate([o[c] for o in emitted]) for c in range(5)]
    want, valid = ref.window_rows(cols, 2, [(1, True)], "rank", limit=3)
    assert all(valid)
    assert sorted(got) == sorted(want)
    assert len(want) > 100
    per_window = {}
    for r in want:
        per_window[(r[4], r[2])] = per_window.get((r[4], r[2]), 0) + 1
    assert max(per_window.values()) > 3, "some window's ties go past 3 rows"
