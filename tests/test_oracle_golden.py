"""Pin the C oracle (oracle/arroyo_oracle.c) against the reference's own
golden test vectors (tests/golden/, from arroyo-sql-testing).  These four
queries exercise the exact operators on the hot path: sliding (q5 window
parameters hop 2s/10s), keyed sliding (hop 1min/1h GROUP BY driver_id),
tumbling keyed/unkeyed, and both watermark-lateness variants."""
import os

import numpy as np
import pytest

import oracle
from arroyo_amd import cabi
from arroyo_amd.pipeline import (NS, batches_from_columns, concat_outputs,
                                 run_stream)
from tests.golden_util import assert_rows_match, fmt_ts, load_golden, load_inputs


def make_oracle(**kw):
    return oracle.make_op(cabi.make_config(**kw))


def test_sliding_window_end():
    # sliding_window_end.sql: hop(2s, 10s), COUNT(*), MIN(counter),
    # MAX(counter) over impulse.json, unkeyed; default 1s watermark lateness.
    inp = load_inputs()["impulse"]
    ts = np.array(inp["ts"], dtype=np.int64)
    counter = np.array(inp["counter"], dtype=np.int64)
    op = make_oracle(width_ns=10 * NS, slide_ns=2 * NS, n_keys=0,
                     n_value_cols=1,
                     aggs=[(cabi.COUNT, -1), (cabi.MIN, 0), (cabi.MAX, 0)])
    outs = run_stream(op, batches_from_columns([counter, ts], 32), NS)
    cols = concat_outputs(outs)
    cnt, mn, mx, ws, we, _ = cols
    got = [{"count": int(c), "min": int(a), "max": int(b),
            "start": fmt_ts(s), "end": fmt_ts(e)}
           for c, a, b, s, e in zip(cnt, mn, mx, ws, we)]
    assert_rows_match(got, load_golden("sliding_window_end"))
    op.close()


def test_hourly_by_event_type():
    # hourly_by_event_type.sql: tumble(1h) COUNT GROUP BY event_type over
    # cars.json (string key dictionary-encoded to i64 by the fixture).
    inp = load_inputs()["cars"]
    ts = np.array(inp["ts"], dtype=np.int64)
    key = np.array(inp["event_type_id"], dtype=np.int64)
    names = inp["event_type_dict"]
    op = make_oracle(width_ns=3600 * NS, slide_ns=0, is_tumbling=True,
                     n_keys=1, n_value_cols=0, aggs=[(cabi.COUNT, -1)])
    outs = run_stream(op, batches_from_columns([key, ts], 32), NS)
    k, cnt, ws, we, _ = concat_outputs(outs)
    got = [{"event_type": names[int(kk)], "hour": fmt_ts(s), "count": int(c)}
           for kk, c, s in zip(k, cnt, ws)]
    assert_rows_match(got, load_golden("hourly_by_event_type"))
    op.close()


def test_tight_watermark():
    # tight_watermark.sql: tumble(1h) COUNT, unkeyed, WATERMARK FOR timestamp
    # (zero lateness); sink emits window.end.
    inp = load_inputs()["cars"]
    ts = np.array(inp["ts"], dtype=np.int64)
    op = make_oracle(width_ns=3600 * NS, slide_ns=0, is_tumbling=True,
                     n_keys=0, n_value_cols=0, aggs=[(cabi.COUNT, -1)])
    outs = run_stream(op, batches_from_columns([ts], 32), 0)
    cnt, ws, we, _ = concat_outputs(outs)
    got = [{"count": int(c), "timestamp": fmt_ts(e)} for c, e in zip(cnt, we)]
    assert_rows_match(got, load_golden("tight_watermark"))
    op.close()


def test_month_loose_watermark():
    # month_loose_watermark.sql: tumble(30 days) unkeyed COUNT over cars
    # with `watermark AS (timestamp - INTERVAL '1 minute')` -- one 30-day
    # bin (epoch-aligned: 2023-08-21 = 653 x 30d) holding all 7932 rows.
    inp = load_inputs()["cars"]
    ts = np.array(inp["ts"], dtype=np.int64)
    op = make_oracle(width_ns=30 * 86400 * NS, slide_ns=0, is_tumbling=True,
                     n_keys=0, n_value_cols=0, aggs=[(cabi.COUNT, -1)])
    outs = run_stream(op, batches_from_columns([ts], 32), 60 * NS)
    cnt, ws, we, _ = concat_outputs(outs)
    got = [{"month": fmt_ts(s), "count": int(c)} for c, s in zip(cnt, ws)]
    assert_rows_match(got, load_golden("month_loose_watermark"))
    op.close()


def test_most_active_driver_last_hour():
    # most_active_driver_last_hour.sql: hop(1min, 1h) COUNT GROUP BY
    # driver_id over cars.json, watermark = ts - 1h; the ROW_NUMBER()=1
    # top-per-window reduction is downstream plumbing replicated here.
    inp = load_inputs()["cars"]
    ts = np.array(inp["ts"], dtype=np.int64)
    key = np.array(inp["driver_id"], dtype=np.int64)
    op = make_oracle(width_ns=3600 * NS, slide_ns=60 * NS, n_keys=1,
                     n_value_cols=0, aggs=[(cabi.COUNT, -1)])
    outs = run_stream(op, batches_from_columns([key, ts], 32), 3600 * NS)
    k, cnt, ws, we, _ = concat_outputs(outs)
    best = {}
    for kk, c, s, e in zip(k, cnt, ws, we):
        cur = best.get(int(s))
        if cur is None or (int(c), int(kk)) > (cur[0], cur[1]):
            best[int(s)] = (int(c), int(kk), int(e))
    got = [{"count": c, "driver_id": d, "end": fmt_ts(e), "row_number": 1,
            "start": fmt_ts(s)}
           for s, (c, d, e) in best.items()]
    assert_rows_match(got, load_golden("most_active_driver_last_hour"))
    op.close()


def _pyoracle_run(width, slide, is_tumbling, key_col, aggs, cols, lateness,
                  batch):
    from oracle import pyoracle as po
    rows = list(zip(*[c.tolist() for c in cols]))
    agg = po.Agg([(op_, c) for op_, c in aggs])
    if is_tumbling:
        op = po.TumblingWindow(width, (0,) if key_col else (), agg)
    else:
        op = po.SlidingWindow(width, slide, (0,) if key_col else (), agg)
    # pyoracle rows: key (if any) is col 0; Agg col indices address the full
    # row tuple, so shift by n_keys
    agg.specs = [(o, (c + (1 if key_col else 0)) if c >= 0 else -1)
                 for o, c in aggs]
    return po.run_pipeline(rows, op, lateness, batch)


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
@pytest.mark.parametrize("tumbling", [False, True])
def test_c_oracle_vs_pyoracle_fuzz(seed, tumbling):
    """Property fuzz: randomized small streams incl. out-of-order data (late
    drops), gaps larger than the window, duplicate timestamps, and bin
    boundaries; C oracle must match the pure-Python restatement exactly."""
    rng = np.random.default_rng(seed)
    n = 3000
    width, slide = 10 * NS, 2 * NS
    # mostly-monotone timestamps with jitter and occasional large gaps
    base = np.cumsum(rng.integers(0, 50_000_000, size=n))
    jitter = rng.integers(-2 * NS, 2 * NS, size=n)
    gaps = (rng.random(n) < 0.002) * rng.integers(0, 60 * NS, size=n)
    ts = np.maximum(100 * NS + base + jitter + np.cumsum(gaps), 0).astype(np.int64)
    key = rng.integers(0, 37, size=n).astype(np.int64)
    val = rng.integers(-1000, 1000, size=n).astype(np.int64)
    aggs = [(cabi.COUNT, -1), (cabi.SUM, 0), (cabi.MIN, 0), (cabi.MAX, 0)]
    cop = make_oracle(width_ns=width, slide_ns=slide, is_tumbling=tumbling,
                      n_keys=1, n_value_cols=1, aggs=aggs)
    outs = run_stream(cop, batches_from_columns([key, val, ts], 97), NS)
    cols = concat_outputs(outs)
    got = set()
    if cols is not None:
        for r in range(len(cols[0])):
            got.add(tuple(int(c[r]) for c in cols))
    want = set()
    for (k, fin, ws, we, ots) in _pyoracle_run(
            width if not tumbling else width, slide, tumbling, True,
            aggs, [key, val, ts], NS, 97):
        want.add((k[0], *[int(x) for x in fin], ws, we, ots))
    assert got == want
    cop.close()


@pytest.mark.parametrize("seed", [11, 13])
def test_c_oracle_avg_fuzz(seed):
    """Same property fuzz with AVG in the agg set (f64 output column).
    The C oracle and the pure-Python restatement both accumulate the AVG
    partial as an IEEE double in arrival order, so values match to 1e-12
    relative (1e-9 is the stated cross-device bar)."""
    rng = np.random.default_rng(seed)
    n = 2000
    width, slide = 10 * NS, 2 * NS
    base = np.cumsum(rng.integers(0, 50_000_000, size=n))
    ts = (100 * NS + base).astype(np.int64)
    key = rng.integers(0, 23, size=n).astype(np.int64)
    val = rng.integers(-1000, 1000, size=n).astype(np.int64)
    aggs = [(cabi.COUNT, -1), (cabi.AVG, 0)]
    cop = make_oracle(width_ns=width, slide_ns=slide, n_keys=1,
                      n_value_cols=1, aggs=aggs)
    outs = run_stream(cop, batches_from_columns([key, val, ts], 89), NS)
    cols = concat_outputs(outs)
    got = {}
    for r in range(len(cols[0])):
        # key, count, avg(f64), window_start, window_end, ts
        kk = (int(cols[0][r]), int(cols[1][r]), int(cols[3][r]),
              int(cols[4][r]), int(cols[5][r]))
        got[kk] = float(cols[2][r])
    want = {}
    for (k, fin, ws, we, ots) in _pyoracle_run(
            width, slide, False, True, aggs, [key, val, ts], NS, 89):
        want[(k[0], int(fin[0]), ws, we, ots)] = float(fin[1])
    assert set(got) == set(want)
    for kk, av in want.items():
        assert got[kk] == pytest.approx(av, rel=1e-12)
    assert len(want) > 500
    cop.close()


def test_golden_fixtures_reproducible(tmp_path):
    """Re-running the extraction must reproduce the committed fixtures
    bit-for-bit (guards against fixture drift).  Its source is staged from
    the repository alone, in the reference's layout: the raw input files
    (kept xz-compressed under tests/golden/raw/inputs/, from which
    inputs.json is derived) and the golden outputs, which the fixtures hold row for row
    and the extraction only re-encodes."""
    import json
    import lzma
    import shutil
    import subprocess
    import sys
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    committed = os.path.join(repo, "tests", "golden")
    names = sorted(n for n in os.listdir(committed) if n.endswith(".json"))
    ref, out = tmp_path / "ref", tmp_path / "out"
    raw = os.path.join(committed, "raw", "inputs")
    os.makedirs(ref / "inputs")
    os.makedirs(ref / "golden_outputs")
    for n in os.listdir(raw):                      # <name>.json.xz
        with lzma.open(os.path.join(raw, n)) as src, \
                open(ref / "inputs" / n[:-len(".xz")], "wb") as dst:
            shutil.copyfileobj(src, dst)
    suffix = ".golden.json"
    for n in names:
        if not n.endswith(suffix):
            continue
        with open(os.path.join(committed, n)) as f:
            rows = json.load(f)
        with open(ref / "golden_outputs" / (n[:-len(suffix)] + ".json"),
                  "w") as f:
            f.writelines(json.dumps(r) + "\n" for r in rows)
    env = dict(os.environ, GOLDEN_REF=str(ref), GOLDEN_OUT=str(out))
    subprocess.run([sys.executable, os.path.join(repo, "oracle",
                                                 "gen_golden.py")],
                   check=True, env=env, capture_output=True)
    assert names == sorted(os.listdir(out))
    for n in names:
        with open(os.path.join(committed, n)) as f1, open(out / n) as f2:
            assert json.load(f1) == json.load(f2), n
