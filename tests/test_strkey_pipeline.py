"""Raw string key columns end to end on the GPU: the device string-key
dictionary (arroyo_amd_strkey_*) in front of, and behind, the existing
int64-keyed operators.  The host never maps a string to an id on the GPU
side; the checkers are the reference's golden vector, the oracle operator fed
ids from a Python dict, and a Python nested-loop join."""
from collections import Counter

import numpy as np
import pytest

import oracle
from arroyo_amd import cabi
from arroyo_amd.cabi import arrow_to_strings, strings_to_arrow
from arroyo_amd.pipeline import NS, U64MAX, WatermarkGen

pytestmark = pytest.mark.gpu


def run_string_keyed_window(strings, ts, batch, strkey_cfg, win_cfg,
                            lateness=NS):
    """strings_to_arrow -> encode_device -> window op process_batch_device
    per batch, watermarks as pipeline.run_stream generates them; the emitted
    key column is decoded on the way out.  Returns a list of
    (string, agg, window_start, window_end, ts) tuples."""
    import torch
    from arroyo_amd import gpu
    dev = torch.device("cuda", 0)
    sk = gpu.make_strkey(strkey_cfg)
    op = gpu.make_op(win_cfg)
    wg = WatermarkGen(lateness)
    rows = []

    def collect(out):
        if not out or not len(out[0]):
            return
        keys = arrow_to_strings(*sk.decode(out[0]))
        rows.extend(zip(keys, *(c.tolist() for c in out[1:])))

    for lo in range(0, len(ts), batch):
        part = strings[lo:lo + batch]
        n = len(part)
        offsets, data = strings_to_arrow(part)
        t_off = torch.from_numpy(offsets).to(dev)
        t_data = torch.from_numpy(data).to(dev)
        t_ts = torch.from_numpy(ts[lo:lo + n].copy()).to(dev)
        t_ids = torch.empty(n, dtype=torch.int64, device=dev)
        # fence torch's H2D stream before the handles' own streams read
        torch.cuda.synchronize()
        sk.encode_device(t_off.data_ptr(), t_data.data_ptr(), n,
                         t_ids.data_ptr())
        op.process_batch_device([t_ids.data_ptr(), t_ts.data_ptr()], n)
        wm = wg.on_batch(ts[lo:lo + n])
        if wm is not None:
            collect(op.handle_watermark(wm))
    collect(op.handle_watermark(U64MAX))
    op.close()
    sk.close()
    return rows


def test_golden_hourly_by_event_type_from_raw_strings():
    """hourly_by_event_type.sql: tumble(1h) COUNT GROUP BY event_type over
    cars.json, keyed on the raw strings."""
    from tests.golden_util import (assert_rows_match, fmt_ts, load_golden,
                                   load_inputs)
    cars = load_inputs()["cars"]
    ts = np.array(cars["ts"], dtype=np.int64)
    names = cars["event_type_dict"]
    strings = [names[i] for i in cars["event_type_id"]]
    rows = run_string_keyed_window(
        strings, ts, 32,
        cabi.make_strkey_config(log2_capacity=6, arena_bytes=4096),
        cabi.make_config(width_ns=3600 * NS, slide_ns=0, is_tumbling=True,
                         n_keys=1, n_value_cols=0, aggs=[(cabi.COUNT, -1)],
                         log2_capacity=10))
    got = [{"event_type": k.decode(), "hour": fmt_ts(ws), "count": int(c)}
           for k, c, ws, we, _ in rows]
    assert_rows_match(got, load_golden("hourly_by_event_type"))


def test_many_string_keys_match_the_oracle_operator():
    rng = np.random.default_rng(12)
    pool = set()
    while len(pool) < 5000:
        ln = int(rng.integers(0, 41))
        pool.add(rng.integers(0, 256, size=ln, dtype=np.uint8).tobytes())
    pool = sorted(pool)
    n = 50_000
    pick = (rng.zipf(1.3, size=n) - 1) % 5000
    strings = [pool[i] for i in pick]
    ts = 1_600_000_000 * NS + np.sort(
        rng.integers(0, 120 * NS, size=n)).astype(np.int64)
    kw = dict(width_ns=10 * NS, slide_ns=2 * NS, n_keys=1, n_value_cols=0,
              aggs=[(cabi.COUNT, -1)], log2_capacity=14)

    got = run_string_keyed_window(
        strings, ts, 8192,
        cabi.make_strkey_config(log2_capacity=14, arena_bytes=1 << 20),
        cabi.make_config(**kw))

    # checker: the oracle operator fed ids from a Python dict
    ids_of = {}
    ids = np.array([ids_of.setdefault(s, len(ids_of)) for s in strings],
                   dtype=np.int64)
    back = {v: k for k, v in ids_of.items()}
    o = oracle.make_op(cabi.make_config(**kw))
    wg = WatermarkGen(NS)
    want = []

    def collect(out):
        if out and len(out[0]):
            want.extend(zip((back[int(k)] for k in out[0]),
                            *(c.tolist() for c in out[1:])))

    for lo in range(0, n, 8192):
        o.process_batch([ids[lo:lo + 8192], ts[lo:lo + 8192]])
        wm = wg.on_batch(ts[lo:lo + 8192])
        if wm is not None:
            collect(o.handle_watermark(wm))
    collect(o.handle_watermark(U64MAX))
    o.close()

    assert len(want) > 1000
    assert len(got) == len(want)
    assert set(got) == set(want)
    assert len(set(want)) == len(want)


def test_one_dictionary_shared_by_both_sides_of_a_join():
    from arroyo_amd import gpu
    rng = np.random.default_rng(13)
    pool = [b"customer/%03d/%s" % (i, b"x" * (i % 7)) for i in range(200)]
    n = 2000
    t0 = 1_600_000_000 * NS
    left = [pool[i] for i in rng.integers(0, 200, size=n)]
    right = [pool[i] for i in rng.integers(0, 200, size=n)]
    lval = np.arange(n, dtype=np.int64)
    rval = np.arange(n, dtype=np.int64) + 10_000
    ts = np.full(n, t0, dtype=np.int64)

    sk = gpu.make_strkey(cabi.make_strkey_config(log2_capacity=10,
                                                 arena_bytes=1 << 16))
    j = gpu.make_join_op(cabi.make_join_config(n_keys=1, n_left_vals=1,
                                               n_right_vals=1))
    j.process_batch(j.LEFT, [sk.encode(*strings_to_arrow(left)), lval, ts])
    j.process_batch(j.RIGHT, [sk.encode(*strings_to_arrow(right)), rval, ts])
    out = j.handle_watermark(U64MAX)
    j.close()
    assert sk.count() <= 200
    keys = arrow_to_strings(*sk.decode(out[0]))
    sk.close()
    got = Counter(zip(keys, out[1].tolist(), out[2].tolist(),
                      out[3].tolist()))

    want = Counter()
    for li in range(n):
        for ri in range(n):
            if left[li] == right[ri]:
                want[(left[li], int(lval[li]), int(rval[ri]), t0)] += 1
    assert sum(want.values()) > 1000
    assert got == want
