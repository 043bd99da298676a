"""The stable device shuffle (arroyo_amd_shuffle_*) inside sharded pipelines,
one process and one device: the ranks of a W-way job are simulated in a loop,
every shard with its own handles on device 0 (as test_multigpu_cpu.py's
gpu-marked runs put every shard on one device)."""
import numpy as np
import pytest

from arroyo_amd import cabi
from arroyo_amd.cabi import arrow_to_strings, strings_to_arrow
from arroyo_amd.pipeline import NS, U64MAX, WatermarkGen
from arroyo_amd.shuffle import KEY_HASH, KEY_I64

pytestmark = pytest.mark.gpu


def run_sharded_string_keyed_window(strings, ts, W, B, sk_cfg, win_cfg):
    """W sources (round-robin over rounds of W * B rows) and W shards.  Each
    source batch is encoded for its content hashes, split on device in
    KEY_HASH mode with the strings riding along, and segment p is interned
    by shard p's own dictionary straight from the shuffle's device buffers
    (no rebasing) and fed to shard p's window operator.  Watermarks as
    pipeline.run_stream generates them from each round.  Returns the decoded
    emissions and the set of strings every shard's dictionary holds."""
    import torch
    from arroyo_amd import gpu
    dev = torch.device("cuda", 0)
    max_len = max(len(s) for s in strings)
    hasher = [gpu.make_strkey(sk_cfg()) for _ in range(W)]
    shuf = [gpu.make_shuffler(cabi.make_shuffle_config(
        W, 2, key_col=0, key_mode=KEY_HASH, has_utf8=True, max_rows=B,
        max_bytes=B * max_len), bind_output=False) for _ in range(W)]
    dicts = [gpu.make_strkey(sk_cfg()) for _ in range(W)]
    ops = [gpu.make_op(win_cfg()) for _ in range(W)]
    wg = WatermarkGen(NS)
    rows = []

    def collect(p, out):
        if not out or not len(out[0]):
            return
        keys = arrow_to_strings(*dicts[p].decode(out[0]))
        rows.extend(zip(keys, *(c.tolist() for c in out[1:])))

    for lo in range(0, len(ts), W * B):
        hi = min(lo + W * B, len(ts))
        for src in range(W):
            idx = list(range(lo + src, hi, W))      # round-robin sources
            n = len(idx)
            if n == 0:
                continue
            off, data = strings_to_arrow([strings[i] for i in idx])
            t_off = torch.from_numpy(off).to(dev)
            t_data = torch.from_numpy(data).to(dev)
            t_ts = torch.from_numpy(ts[idx]).to(dev)
            t_ids = torch.empty(n, dtype=torch.int64, device=dev)
            t_hash = torch.empty(n, dtype=torch.int64, device=dev)
            torch.cuda.synchronize()
            hasher[src].encode_device(t_off.data_ptr(), t_data.data_ptr(), n,
                                      t_ids.data_ptr(), t_hash.data_ptr())
            out = shuf[src].partition_ptrs(
                [t_hash.data_ptr(), t_ts.data_ptr()], n, t_off.data_ptr(),
                t_data.data_ptr())
            assert out.row_start[W] == n
            for p in range(W):
                r0, r1 = out.row_start[p], out.row_start[p + 1]
                if r1 == r0:
                    continue
                dicts[p].encode_device(out.utf8_offsets + 4 * (r0 + p),
                                       out.utf8_data + out.byte_start[p],
                                       r1 - r0, t_ids.data_ptr())
                ops[p].process_batch_device(
                    [t_ids.data_ptr(), out.cols[1] + 8 * r0], r1 - r0)
                # the ids and the shuffle's buffers are reused right away
                assert gpu.lib().arroyo_amd_sync(ops[p]._h) == 0
        wm = wg.on_batch(ts[lo:hi])
        if wm is not None:
            for p in range(W):
                collect(p, ops[p].handle_watermark(wm))
    for p in range(W):
        collect(p, ops[p].handle_watermark(U64MAX))
    seen = [set(arrow_to_strings(*d.drain()[1:])) for d in dicts]
    for h in hasher + shuf + dicts + ops:
        h.close()
    # no string was seen by two shards, and together they saw every one
    for a in range(W):
        for b in range(a + 1, W):
            assert not (seen[a] & seen[b])
    assert set().union(*seen) == {s if isinstance(s, bytes) else s.encode()
                                  for s in strings}
    return rows, seen


def test_string_keys_sharded_four_ways_match_the_golden():
    """hourly_by_event_type.sql: tumble(1h) COUNT GROUP BY event_type over
    cars.json on the raw strings, 4 sources and 4 shards, 32 rows a round
    (the cadence of the one-shard test in test_strkey_pipeline.py)."""
    from tests.golden_util import (assert_rows_match, fmt_ts, load_golden,
                                   load_inputs)
    cars = load_inputs()["cars"]
    ts = np.array(cars["ts"], dtype=np.int64)
    names = cars["event_type_dict"]
    strings = [names[i] for i in cars["event_type_id"]]
    rows, _ = run_sharded_string_keyed_window(
        strings, ts, 4, 8,
        lambda: cabi.make_strkey_config(log2_capacity=6, arena_bytes=4096),
        lambda: cabi.make_config(
            width_ns=3600 * NS, slide_ns=0, is_tumbling=True, n_keys=1,
            n_value_cols=0, aggs=[(cabi.COUNT, -1)], log2_capacity=10))
    got = [{"event_type": k.decode(), "hour": fmt_ts(ws), "count": int(c)}
           for k, c, ws, we, _ in rows]
    assert_rows_match(got, load_golden("hourly_by_event_type"))


def test_many_string_keys_sharded_four_ways_match_the_oracle():
    """The golden input has a handful of event types; here 300 binary keys
    (empty string and NUL bytes among them) spread over every shard, checked
    against the single-instance oracle fed ids from a Python dict."""
    import oracle
    rng = np.random.default_rng(21)
    pool = {b"", b"\x00", b"\x00\x00"}
    while len(pool) < 300:
        ln = int(rng.integers(1, 41))
        pool.add(rng.integers(0, 256, size=ln, dtype=np.uint8).tobytes())
    pool = sorted(pool)
    n = 20_000
    strings = [pool[i] for i in (rng.zipf(1.3, size=n) - 1) % 300]
    ts = 1_600_000_000 * NS + np.sort(
        rng.integers(0, 60 * NS, size=n)).astype(np.int64)
    kw = dict(width_ns=10 * NS, slide_ns=2 * NS, n_keys=1, n_value_cols=0,
              aggs=[(cabi.COUNT, -1)], log2_capacity=12)
    got, seen = run_sharded_string_keyed_window(
        strings, ts, 4, 1024,
        lambda: cabi.make_strkey_config(log2_capacity=10,
                                        arena_bytes=1 << 16),
        lambda: cabi.make_config(**kw))
    assert all(len(s) > 20 for s in seen)

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

    for lo in range(0, n, 4096):
        o.process_batch([ids[lo:lo + 4096], ts[lo:lo + 4096]])
        wm = wg.on_batch(ts[lo:lo + 4096])
        if wm is not None:
            collect(o.handle_watermark(wm))
    collect(o.handle_watermark(U64MAX))
    o.close()
    assert len(want) > 1000 and len(set(want)) == len(want)
    assert len(got) == len(want)
    assert set(got) == set(want)


def updating_stream(seed, n_keys=50, n_rows=2000):
    """A keyed updating stream: every key appends rows and later retracts
    some of exactly those rows.  Columns [k0, k1, ckey, v0, v1, is_retract]:
    (k0, k1) is the composite key, ckey its single-column form."""
    rng = np.random.default_rng(seed)
    k0 = np.zeros(n_rows, dtype=np.int64)
    k1 = np.zeros(n_rows, dtype=np.int64)
    v0 = np.zeros(n_rows, dtype=np.int64)
    v1 = np.zeros(n_rows, dtype=np.int64)
    retract = np.zeros(n_rows, dtype=np.int64)
    live = {}
    pairs = [(int(a), int(b)) for a, b in
             zip(rng.integers(0, 20, size=n_keys),
                 rng.integers(0, 7, size=n_keys))]
    for i in range(n_rows):
        a, b = pairs[int(rng.integers(0, n_keys))]
        k0[i], k1[i] = a, b
        mine = live.setdefault((a, b), [])
        if mine and rng.random() < 0.4:
            v0[i], v1[i] = mine.pop(int(rng.integers(0, len(mine))))
            retract[i] = 1
        else:
            v0[i], v1[i] = int(rng.integers(-40, 41)), int(rng.integers(0, 9))
            mine.append((int(v0[i]), int(v1[i])))
    return [k0, k1, k0 * 64 + k1, v0, v1, retract]


def rows_of(cols):
    if cols is None or len(cols) == 0 or len(cols[0]) == 0:
        return []
    return sorted(tuple(int(c[r]) for c in cols) for r in range(len(cols[0])))


def test_updating_aggregate_sharded_two_ways_matches_single():
    """Order matters downstream: retractable MIN/MAX and COUNT DISTINCT
    need a key's append before its retraction.  The stream is split 2 ways
    on k0 with every column carried; the union of the shards' flushes
    equals the single-instance flushes, batch by batch."""
    import torch
    from arroyo_amd import gpu
    W, B = 2, 250
    cols = updating_stream(31)
    n = len(cols[0])
    dev = torch.device("cuda", 0)
    aggs = [(cabi.COUNT, -1), (cabi.MIN_RETRACT, 0), (cabi.MAX_RETRACT, 0),
            (cabi.COUNT_DISTINCT, 1)]
    cfg = lambda: cabi.make_updagg_config(aggs, n_keys=1, n_value_cols=2)
    single = gpu.make_updagg_op(cfg())
    shards = [gpu.make_updagg_op(cfg()) for _ in range(W)]
    sh = gpu.make_shuffler(cabi.make_shuffle_config(
        W, 6, key_col=0, key_mode=KEY_I64, max_rows=B))
    nonempty = 0
    keys_on = [set() for _ in range(W)]
    for lo in range(0, n, B):
        batch = [c[lo:lo + B] for c in cols]
        single.process_batch(batch[2:])
        want = rows_of(single.flush())
        part = sh.partition([torch.from_numpy(c.copy()).to(dev)
                             for c in batch])
        got = []
        for p in range(W):
            seg = part.part_cols(p)
            cnt = part.count(p)
            if cnt == 0:
                continue
            # the composite key travelled with its row
            assert torch.equal(seg[0] * 64 + seg[1], seg[2])
            keys_on[p] |= set(seg[2].cpu().tolist())
            shards[p].process_batch_device(
                [s.data_ptr() for s in seg[2:]], cnt)
            got += rows_of(shards[p].flush())
        assert sorted(got) == want
        nonempty += bool(want)
    assert nonempty >= n // B - 1
    assert keys_on[0] and keys_on[1] and not (keys_on[0] & keys_on[1])
    single.close()
    sh.close()
    for s in shards:
        s.close()
