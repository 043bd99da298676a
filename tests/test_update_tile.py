"""k_update_tile (ARROYO_AMD_UPD=tile, the default update kernel for the
keyed single-COUNT shape) against the CPU oracle, bit-exact, on the shapes
where a per-block LDS table over a contiguous row span can go wrong: partial
sub-tiles and spans, table overflow, a full probe bucket, a pane boundary
inside a tile, sentinel keys and late rows.  Every case also runs with
ARROYO_AMD_UPD=batch (k_update_batch_n) and ARROYO_AMD_UPD=lds
(k_update_lds_vec / k_update_lds) on the same steps."""
import functools

import numpy as np
import pytest

import oracle
from arroyo_amd import cabi, nexmark
from arroyo_amd.pipeline import NS, U64MAX

pytestmark = pytest.mark.gpu

T0 = 1_600_000_000 * NS          # a multiple of the 2 s slide
SLIDE = 2 * NS
RING_PANES = 16
UPD = ["tile", "batch", "lds"]


def config(log2_capacity):
    return cabi.make_config(width_ns=10 * NS, slide_ns=SLIDE, n_keys=1,
                            n_value_cols=0, aggs=[(cabi.COUNT, -1)],
                            log2_capacity=log2_capacity,
                            ring_panes=RING_PANES)


def drive(op, steps):
    """steps: ("batch", [key, ts]) or ("wm", value); a final u64::MAX
    watermark closes every window.  Returns the emitted columns."""
    outs = []
    for kind, arg in list(steps) + [("wm", U64MAX)]:
        if kind == "batch":
            op.process_batch(arg)
        else:
            out = op.handle_watermark(arg)
            if out and len(out[0]):
                outs.append(out)
    if not outs:
        return None
    return [np.concatenate([o[i] for o in outs]) for i in range(len(outs[0]))]


def sorted_rows(cols):
    order = np.lexsort(tuple(cols[::-1]))
    return np.stack([c[order] for c in cols])


def assert_same(got, want):
    assert (got is None) == (want is None)
    if got is None:
        return
    assert len(got[0]) == len(want[0]), (len(got[0]), len(want[0]))
    assert np.array_equal(sorted_rows(got), sorted_rows(want))


def oracle_rows(steps, log2_capacity):
    o = oracle.make_op(config(log2_capacity))
    want = drive(o, steps)
    o.close()
    return want


def gpu_rows(steps, log2_capacity):
    from arroyo_amd import gpu
    g = gpu.make_op(config(log2_capacity))
    got = drive(g, steps)
    g.close()
    return got


def check(case, upd, monkeypatch, blocks=None):
    steps, log2_capacity, want = case
    monkeypatch.setenv("ARROYO_AMD_UPD", upd)
    if blocks is not None:
        monkeypatch.setenv("ARROYO_AMD_BLOCKS", str(blocks))
    assert_same(gpu_rows(steps, log2_capacity), want)


def make_case(steps, log2_capacity):
    return steps, log2_capacity, oracle_rows(steps, log2_capacity)


# -- the kernel's LDS hash, restated in numpy ------------------------------

def hash64(x):
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9e3779b97f4a7c15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xbf58476d1ce4e5b9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94d049bb133111eb)
        return x ^ (x >> np.uint64(31))


def lds_home(key, pane, slots):
    with np.errstate(over="ignore"):
        x = key.astype(np.uint64) * np.uint64(2654435761) + np.uint64(pane)
    return (hash64(x) & np.uint64(slots - 1)).astype(np.int64)


# -- cases (oracle result computed once, shared by all kernels) ------------

@functools.lru_cache(maxsize=None)
def case_odd_rows(n):
    key, ts = nexmark.bids(n, events_per_sec=2000, seed=11)
    return make_case([("batch", [key, ts])], 12)


@functools.lru_cache(maxsize=None)
def case_forced_blocks():
    # 10,007 rows = 5 sub-tiles of 2048 rows (the last partial) + 7 tail rows
    key, ts = nexmark.bids(10_007, events_per_sec=2000, seed=12)
    return make_case([("batch", [key, ts])], 12)


@functools.lru_cache(maxsize=None)
def case_overflow(twice):
    """2048 distinct keys in one pane: more than any LDS table holds.  With
    `twice`, a second 2048-row sub-tile repeats every key (other order)."""
    rng = np.random.default_rng(13)
    key = rng.permutation(2048).astype(np.int64) + 5000
    if twice:
        key = np.concatenate([key, rng.permutation(key)])
    ts = T0 + np.arange(len(key), dtype=np.int64) * 1000
    return make_case([("batch", [key, ts])], 13)


@functools.lru_cache(maxsize=None)
def case_full_bucket():
    """12 keys that share one LDS home slot (for every table size up to
    2048 slots, so for every probe limit the kernel is built with), 5 rows
    each, interleaved: the bucket fills and the extras spill."""
    pane = (T0 // SLIDE) & (RING_PANES - 1)
    cand = np.arange(1, 400_000, dtype=np.int64)
    home = lds_home(cand, pane, 2048)
    same = cand[home == home[0]][:12]
    assert len(same) == 12
    key = np.tile(same, 5)
    ts = T0 + np.arange(len(key), dtype=np.int64) * 1000
    return make_case([("batch", [key, ts])], 12)


@functools.lru_cache(maxsize=None)
def case_pane_boundary():
    """One key; the tile's timestamps cross the slide boundary at T0 + 2 s
    after 1000 of its 2048 rows."""
    n = 2048
    key = np.full(n, 77, dtype=np.int64)
    ts = T0 + SLIDE + (np.arange(n, dtype=np.int64) - 1000) * 1000
    return make_case([("batch", [key, ts])], 12)


@functools.lru_cache(maxsize=None)
def case_sentinel():
    rng = np.random.default_rng(14)
    n = 5000
    key = rng.choice(np.array([-1, 5, 7, 9], dtype=np.int64), size=n)
    ts = T0 + np.arange(n, dtype=np.int64) * 1_000_000
    return make_case([("batch", [key, ts])], 12)


@functools.lru_cache(maxsize=None)
def case_late_rows():
    """After the watermark T0 + 5 s (cutoff bin T0 + 4 s) one 2048-row tile
    mixes rows of the panes T0 and T0 + 2 s, which are late and dropped,
    with live rows of T0 + 4 s and T0 + 6 s."""
    rng = np.random.default_rng(15)
    k1 = rng.integers(0, 50, size=3000).astype(np.int64)
    t1 = T0 + np.sort(rng.integers(0, 6 * NS, size=3000)).astype(np.int64)
    k2 = rng.integers(0, 50, size=2048).astype(np.int64)
    t2 = T0 + rng.integers(0, 8 * NS, size=2048).astype(np.int64)
    return make_case([("batch", [k1, t1]), ("wm", T0 + 5 * NS),
                      ("batch", [k2, t2])], 12)


# -- tests -----------------------------------------------------------------

@pytest.mark.parametrize("upd", UPD)
@pytest.mark.parametrize("n", [1, 7, 2047, 2049, 3 * 2048 + 5])
def test_odd_row_counts(n, upd, monkeypatch):
    check(case_odd_rows(n), upd, monkeypatch)


@pytest.mark.parametrize("upd", UPD)
@pytest.mark.parametrize("blocks", [1, 3])
def test_forced_block_counts(blocks, upd, monkeypatch):
    check(case_forced_blocks(), upd, monkeypatch, blocks=blocks)


# the lds kernel has no rows-per-thread knob, so it has no case here
@pytest.mark.parametrize("upd", ["tile", "batch"])
@pytest.mark.parametrize("bq", [12, 16])
def test_wider_rows_per_thread(bq, upd, monkeypatch):
    # ARROYO_AMD_BQ keeps its meaning under both kernels; 10,007 rows leave
    # a partial sub-tile and a tail for either width
    monkeypatch.setenv("ARROYO_AMD_BQ", str(bq))
    check(case_forced_blocks(), upd, monkeypatch)


@pytest.mark.parametrize("upd", UPD)
def test_lds_overflow(upd, monkeypatch):
    check(case_overflow(False), upd, monkeypatch)


@pytest.mark.parametrize("upd", UPD)
def test_lds_overflow_every_key_twice(upd, monkeypatch):
    # one block, so the second sub-tile meets the table the first one filled
    check(case_overflow(True), upd, monkeypatch, blocks=1)


@pytest.mark.parametrize("upd", UPD)
def test_full_bucket(upd, monkeypatch):
    check(case_full_bucket(), upd, monkeypatch)


@pytest.mark.parametrize("upd", UPD)
def test_pane_boundary_inside_tile(upd, monkeypatch):
    case = case_pane_boundary()
    check(case, upd, monkeypatch)
    # the oracle's own result, pinned: 1000 rows in pane T0, 1048 in T0 + 2 s
    want = sorted_rows(case[2])
    first = want[:, want[2] == T0 - 8 * NS]      # window [T0 - 8 s, T0 + 2 s)
    assert first.shape[1] == 1 and first[1, 0] == 1000
    full = want[:, want[2] == T0]                # window [T0, T0 + 10 s)
    assert full.shape[1] == 1 and full[1, 0] == 2048


@pytest.mark.parametrize("upd", UPD)
def test_sentinel_rows(upd, monkeypatch):
    check(case_sentinel(), upd, monkeypatch)


@pytest.mark.parametrize("upd", UPD)
def test_late_rows(upd, monkeypatch):
    check(case_late_rows(), upd, monkeypatch)


@functools.lru_cache(maxsize=None)
def case_multi_batch():
    key, ts = nexmark.bids(4 * 4096, events_per_sec=2000, seed=16)
    off = 6 * NS + 12345
    want = oracle_rows([("batch", [key, ts + off])], 14)
    return key, ts, off, want


@pytest.mark.parametrize("upd", UPD)
def test_multi_batch_device_submission(upd, monkeypatch):
    """The bench's submit path: process_batches_device(contiguous=True) with
    n_batches > 1 and a non-zero ts_offset0."""
    import torch

    from arroyo_amd import gpu

    key, ts, off, want = case_multi_batch()
    monkeypatch.setenv("ARROYO_AMD_UPD", upd)
    dev = torch.device("cuda", 0)
    d_key = torch.from_numpy(key).to(dev)
    d_ts = torch.from_numpy(ts).to(dev)
    g = gpu.make_op(config(14))
    g.process_batches_device([d_key.data_ptr(), d_ts.data_ptr()], 4096, 4,
                             contiguous=True, ts_offset0=off)
    got = drive(g, [])
    assert g.perf()["rows"] == 4 * 4096
    g.close()
    assert_same(got, want)
