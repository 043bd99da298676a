"""Composite and NULL keys end to end on the GPU: the device tuple-key
dictionary (arroyo_amd_tuplekey_*) in front of, and behind, the unchanged
single-key operators.  The host never maps a tuple to an id on the GPU side;
the checker is the CPU oracle operator keyed on ids that a Python dict
assigns to the same tuples (or a plain Python model), and the two sides are
compared as (decoded tuple, values) rows, since the ids differ."""
import numpy as np
import pytest

import oracle
from arroyo_amd import cabi
from arroyo_amd.cabi import arrow_to_strings, strings_to_arrow
from arroyo_amd.pipeline import NS, U64MAX
from arroyo_amd.shuffle import KEY_HASH, tuple_hash_np

pytestmark = pytest.mark.gpu

HOUR = 3600 * NS


def rows_of(cols):
    if cols is None or len(cols) == 0 or len(cols[0]) == 0:
        return []
    return [tuple(int(c[r]) for c in cols) for r in range(len(cols[0]))]


def fold(state, emissions):
    """Merge an updating aggregate's (key, vals..., is_retract) emissions
    into the state they describe: a retract removes exactly the current
    value of its key, an append sets it."""
    for key, *vals, retract in emissions:
        if retract:
            assert state.pop(key) == tuple(vals), f"stale retract for {key}"
        else:
            assert key not in state, f"append over live key {key}"
            state[key] = tuple(vals)
    return state


class DictIds:
    """The checker's interner: a Python dict."""

    def __init__(self):
        self.ids, self.back = {}, []

    def encode(self, keys):
        out = []
        for k in keys:
            if k not in self.ids:
                self.ids[k] = len(self.back)
                self.back.append(k)
            out.append(self.ids[k])
        return np.array(out, dtype=np.int64)


def decode_tuples(tk, ids):
    """ids -> list of tuples, a NULL component as None"""
    cols, masks = tk.decode(np.asarray(ids, dtype=np.int64))
    out = []
    for r in range(len(ids)):
        out.append(tuple(
            None if masks is not None and masks[c] is not None
            and not masks[c][r] else int(cols[c][r])
            for c in range(len(cols))))
    return out


def test_updating_aggregate_group_by_event_type_and_driver_id():
    """SELECT event_type, driver_id, COUNT(*), SUM(second_of_hour) FROM cars
    GROUP BY event_type, driver_id on the raw strings: strkey, tuplekey over
    (string id, driver_id), updagg, tuplekey decode, strkey decode."""
    from arroyo_amd import gpu
    from tests.golden_util import load_inputs
    cars = load_inputs()["cars"]
    names = cars["event_type_dict"]
    strings = [names[i].encode() for i in cars["event_type_id"]]
    driver = np.array(cars["driver_id"], dtype=np.int64)
    val = np.array(cars["ts"], dtype=np.int64) // NS % 3600
    n = len(driver)
    aggs = [(cabi.COUNT, -1), (cabi.SUM, 0)]
    cfg = lambda: cabi.make_updagg_config(aggs, n_keys=1, n_value_cols=1,
                                          log2_capacity=10)
    zeros = np.zeros(n, dtype=np.int64)

    sk = gpu.make_strkey(cabi.make_strkey_config(log2_capacity=6,
                                                 arena_bytes=4096))
    tk = gpu.make_tuplekey(cabi.make_tuplekey_config(2, log2_capacity=10))
    g = gpu.make_updagg_op(cfg())
    o = oracle.make_updagg_op(cfg())
    ref = DictIds()
    got_state, want_state = {}, {}
    for lo in range(0, n, 1000):
        sl = slice(lo, lo + 1000)
        sid = sk.encode(*strings_to_arrow(strings[sl]))
        ids = tk.encode([sid, driver[sl]])
        g.process_batch([ids, val[sl], zeros[sl]])
        fold(got_state, rows_of(g.flush()))
        o.process_batch([ref.encode(zip(strings[sl], driver[sl].tolist())),
                         val[sl], zeros[sl]])
        fold(want_state, rows_of(o.flush()))
    g.close()
    o.close()

    keys = list(got_state)
    tuples = decode_tuples(tk, keys)
    event = arrow_to_strings(*sk.decode(
        np.array([t[0] for t in tuples], dtype=np.int64)))
    got = {(e, t[1]) + got_state[k] for e, t, k in zip(event, tuples, keys)}
    assert len(got) == len(keys) == tk.count()
    assert sk.count() == len(names)
    sk.close()
    tk.close()

    want = {ref.back[k] + v for k, v in want_state.items()}
    plain = {}
    for s, d, v in zip(strings, driver.tolist(), val.tolist()):
        c, t = plain.get((s, d), (0, 0))
        plain[(s, d)] = (c + 1, t + v)
    assert got == want
    assert got == {k + v for k, v in plain.items()}
    assert len(got) > 150 and len({k[0] for k in got}) == len(names)


def test_two_column_equi_join_through_expjoin():
    """JOIN ... ON l.x = r.x AND l.y = r.y: both sides encode on one shared
    handle.  (1, 2) and (2, 1), (0, 3) and (3, 0) are among the pairs."""
    from arroyo_amd import gpu
    rng = np.random.default_rng(71)
    pairs = [(x, y) for x in range(7) for y in range(7)]
    assert (1, 2) in pairs and (2, 1) in pairs
    t0 = 1_600_000_000 * NS
    cfg = lambda: cabi.make_expjoin_config(24 * HOUR, n_left_vals=1,
                                           n_right_vals=1, log2_capacity=10,
                                           log2_rows_cap=12)
    tk = gpu.make_tuplekey(cabi.make_tuplekey_config(2, log2_capacity=10))
    g = gpu.make_expjoin_op(cfg())
    o = oracle.make_expjoin_op(cfg())
    ref = DictIds()
    got, want = [], []
    for step in range(4):
        n = 300
        pick = rng.integers(0, len(pairs), size=n)
        x = np.array([pairs[i][0] for i in pick], dtype=np.int64)
        y = np.array([pairs[i][1] for i in pick], dtype=np.int64)
        v = rng.integers(0, 10**6, size=n).astype(np.int64)
        ts = t0 + (step * 60 + np.sort(
            rng.integers(0, 60, size=n))).astype(np.int64) * NS
        side = step % 2
        out = rows_of(g.process_batch(side, [tk.encode([x, y]), v, ts]))
        for r, t in zip(out, decode_tuples(tk, [r[0] for r in out])):
            got.append(t + r[1:])
        out = rows_of(o.process_batch(
            side, [ref.encode(zip(x.tolist(), y.tolist())), v, ts]))
        want += [ref.back[r[0]] + r[1:] for r in out]
    g.close()
    o.close()
    assert tk.count() == len(ref.back) <= 49
    tk.close()
    assert len(want) > 1000
    assert sorted(got) == sorted(want)
    assert {r[:2] for r in got} >= {(1, 2), (2, 1), (0, 3), (3, 0)}


def test_group_by_a_nullable_column_puts_all_nulls_in_one_group():
    """GROUP BY k with k NULL on about a fifth of the rows: a nullable
    tuplekey handle in front of the updating aggregate's nullable surface.
    The value column is nullable too, so SUM skips its NULLs."""
    from arroyo_amd import gpu
    rng = np.random.default_rng(72)
    n = 3000
    key = rng.integers(0, 40, size=n).astype(np.int64)
    kvalid = rng.random(n) >= 0.2
    key = np.where(kvalid, key, rng.integers(-10**9, 10**9, size=n))
    val = rng.integers(-100, 100, size=n).astype(np.int64)
    vvalid = rng.random(n) >= 0.3
    zeros = np.zeros(n, dtype=np.int64)
    assert 0.15 < 1 - kvalid.mean() < 0.25

    tk = gpu.make_tuplekey(cabi.make_tuplekey_config(1, log2_capacity=10,
                                                     nullable=True))
    g = gpu.make_updagg_op(cabi.make_updagg_config(
        [(cabi.COUNT, -1), (cabi.SUM, 0)], n_keys=1, n_value_cols=1,
        log2_capacity=10, null_semantics=True))
    for lo in range(0, n, 1000):
        sl = slice(lo, lo + 1000)
        ids = tk.encode([key[sl]], [kvalid[sl]])
        g.process_batch_nullable([ids, val[sl], zeros[sl]],
                                 [None, vvalid[sl], None])
    cols, masks = g.flush_with_validity()
    g.close()
    assert not cols[-1].any(), "one flush of fresh keys: appends only"
    kcols, kmasks = tk.decode(cols[0])
    assert tk.count() == 41
    tk.close()
    # exactly one group is the NULL group: validity bit clear, value 0
    assert kmasks is not None and (~kmasks[0]).sum() == 1
    assert kcols[0][~kmasks[0]].tolist() == [0]
    got = {}
    for r in range(len(cols[0])):
        k = int(kcols[0][r]) if kmasks[0][r] else None
        assert k not in got
        got[k] = (int(cols[1][r]),
                  int(cols[2][r]) if masks[2][r] else None)

    want = {}
    for k, kv, v, vv in zip(key.tolist(), kvalid.tolist(), val.tolist(),
                            vvalid.tolist()):
        k = k if kv else None
        c, s = want.get(k, (0, None))
        want[k] = (c + 1, (s or 0) + v if vv else s)
    assert got == want
    assert got[None][0] == int((~kvalid).sum())


def test_rank_partition_by_two_columns():
    """RANK() OVER (PARTITION BY window, region ORDER BY score DESC): the
    window-function operator partitions on the tuple's id; the function
    values are those of tests/windowfn_ref.py run on dict ids."""
    from arroyo_amd import gpu
    from tests import windowfn_ref as ref
    rng = np.random.default_rng(73)
    n = 600
    t0 = 1_600_000_000 * NS
    window = rng.integers(1, 4, size=n).astype(np.int64)
    region = rng.integers(1, 4, size=n).astype(np.int64)   # (1, 2), (2, 1)..
    score = rng.integers(0, 12, size=n).astype(np.int64)   # many ties
    ts = t0 + rng.integers(0, 3, size=n).astype(np.int64) * NS

    tk = gpu.make_tuplekey(cabi.make_tuplekey_config(2, log2_capacity=10))
    wf = gpu.make_windowfn_op(cabi.make_windowfn_config(
        n_cols=3, part_col=0, order=[(1, True)], log2_rows_cap=12,
        fn=cabi.WFN_RANK))
    for lo in range(0, n, 200):
        sl = slice(lo, lo + 200)
        wf.process_batch([tk.encode([window[sl], region[sl]]), score[sl],
                          ts[sl]])
    out = rows_of(wf.handle_watermark(U64MAX))
    wf.close()
    got = [t + r[1:] for r, t in
           zip(out, decode_tuples(tk, [r[0] for r in out]))]
    assert tk.count() == 9
    tk.close()

    ids = DictIds()
    pid = ids.encode(zip(window.tolist(), region.tolist()))
    rows, valid = ref.window_rows([pid, score, ts], 0, [(1, True)], "rank")
    assert all(valid)
    want = [ids.back[r[0]] + r[1:] for r in rows]
    assert len(want) == n
    assert sorted(got) == sorted(want)
    assert max(r[-1] for r in want) > 5


def test_sharded_two_ways_on_the_tuple_hash():
    """The sender hashes the raw tuples (tuple_hash_np, what
    tuplekey_hash_device computes), the shuffle splits in KEY_HASH mode with
    the components riding along, and every shard interns what it receives in
    a dictionary of its own.  The union of the shards' decoded flushes equals
    the unsharded run."""
    import torch
    from arroyo_amd import gpu
    rng = np.random.default_rng(74)
    W, B, n = 2, 500, 2000
    dev = torch.device("cuda", 0)
    a = rng.integers(0, 12, size=n).astype(np.int64)
    b = rng.integers(0, 12, size=n).astype(np.int64)
    val = rng.integers(-50, 50, size=n).astype(np.int64)
    h = tuple_hash_np([a, b]).view(np.int64)
    aggs = [(cabi.COUNT, -1), (cabi.SUM, 0)]
    ucfg = lambda: cabi.make_updagg_config(aggs, n_keys=1, n_value_cols=1,
                                           log2_capacity=10)
    tcfg = lambda: cabi.make_tuplekey_config(2, log2_capacity=10)

    single_tk, single = gpu.make_tuplekey(tcfg()), gpu.make_updagg_op(ucfg())
    tks = [gpu.make_tuplekey(tcfg()) for _ in range(W)]
    shards = [gpu.make_updagg_op(ucfg()) for _ in range(W)]
    sh = gpu.make_shuffler(cabi.make_shuffle_config(
        W, 4, key_col=0, key_mode=KEY_HASH, max_rows=B))
    t_ids = torch.empty(B, dtype=torch.int64, device=dev)
    t_zero = torch.zeros(B, dtype=torch.int64, device=dev)
    want_state, got_state = {}, [{} for _ in range(W)]
    for lo in range(0, n, B):
        sl = slice(lo, lo + B)
        single.process_batch([single_tk.encode([a[sl], b[sl]]), val[sl],
                              np.zeros(B, dtype=np.int64)])
        fold(want_state, rows_of(single.flush()))
        part = sh.partition([torch.from_numpy(c[sl].copy()).to(dev)
                             for c in (h, a, b, val)])
        for p in range(W):
            cnt = part.count(p)
            if cnt == 0:
                continue
            seg = part.part_cols(p)
            tks[p].encode_device([seg[1].data_ptr(), seg[2].data_ptr()],
                                 None, cnt, t_ids.data_ptr())
            shards[p].process_batch_device(
                [t_ids.data_ptr(), seg[3].data_ptr(), t_zero.data_ptr()],
                cnt)
            # flush synchronises: the ids and the shuffle's buffers are
            # reused by the next round
            fold(got_state[p], rows_of(shards[p].flush()))

    def decoded(tk, state):
        keys = list(state)
        return {t + state[k] for t, k in zip(decode_tuples(tk, keys), keys)}

    want = decoded(single_tk, want_state)
    got = [decoded(tks[p], got_state[p]) for p in range(W)]
    for handle in [single_tk, single, sh] + tks + shards:
        handle.close()
    assert len(want) > 100
    keys_on = [{r[:2] for r in g} for g in got]
    assert keys_on[0] and keys_on[1] and not (keys_on[0] & keys_on[1])
    assert got[0] | got[1] == want
    assert len(got[0]) + len(got[1]) == len(want)
