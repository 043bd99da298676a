"""Device tuple-key dictionary (arroyo_amd_tuplekey_*): an interner for
composite and nullable keys.  The checker throughout is a Python dict keyed
on (null mask, tuple of words with 0 under a NULL): equal keys must get equal
ids, different keys different ids, and decode must give the key back.  Ids
are opaque; nothing here assumes their values or density, only id >= 0."""
import ctypes
import os
import re

import numpy as np
import pytest

from arroyo_amd import cabi
from arroyo_amd.shuffle import splitmix64_np, tuple_hash_np

gpu_only = pytest.mark.gpu

I64_MIN, I64_MAX = -2**63, 2**63 - 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make_dict(n_cols, **kw):
    from arroyo_amd import gpu
    kw.setdefault("log2_capacity", 10)
    return gpu.make_tuplekey(cabi.make_tuplekey_config(n_cols, **kw))


def columns(rows, n_cols):
    """list of n_cols-tuples -> n_cols int64 columns"""
    a = np.array(rows, dtype=np.int64).reshape(len(rows), n_cols)
    return [np.ascontiguousarray(a[:, c]) for c in range(n_cols)]


def keys_of(cols, valid=None):
    """The checker's key per row: (mask, words with 0 under a NULL)."""
    mask = np.zeros(len(cols[0]), dtype=np.int64)
    words = []
    for c, col in enumerate(cols):
        w = np.asarray(col).view(np.int64)
        if valid is not None and valid[c] is not None:
            null = ~np.asarray(valid[c], dtype=bool)
            mask |= null.astype(np.int64) << c
            w = np.where(null, 0, w)
        words.append(w.tolist())
    return list(zip(mask.tolist(), zip(*words)))


def assert_bijection(keys, ids):
    """ids[i] == ids[j] iff keys[i] == keys[j], and every id >= 0."""
    assert len(keys) == len(ids)
    assert (np.asarray(ids) >= 0).all()
    by_key, by_id = {}, {}
    for k, i in zip(keys, np.asarray(ids).tolist()):
        assert by_key.setdefault(k, i) == i, f"{k!r} got two ids"
        assert by_id.setdefault(i, k) == k, \
            f"id {i} given to {by_id[i]!r} and {k!r}"
    return by_key


def decoded_keys(d, ids):
    """decode(ids) as checker keys; the value under a NULL must be 0."""
    cols, masks = d.decode(ids)
    assert len(cols) == d.cfg.n_cols
    valid = None
    if masks is not None:
        assert len(masks) == d.cfg.n_cols
        valid = masks
        for c, m in zip(cols, masks):
            if m is not None:
                assert m.dtype == bool and len(m) == len(ids)
                assert (c[~m] == 0).all(), "value under a NULL is 0"
    return keys_of(cols, valid)


def shuffled(rows, seed, times=3):
    rng = np.random.default_rng(seed)
    rows = list(rows) * times
    return [rows[i] for i in rng.permutation(len(rows))]


def random_tuples(rng, n, n_cols, lo=-50, hi=50):
    """n distinct random tuples of small words (many shared components)."""
    seen = set()
    while len(seen) < n:
        seen.add(tuple(int(x) for x in rng.integers(lo, hi, size=n_cols)))
    return sorted(seen)


# ---- 1. CPU -----------------------------------------------------------------

def test_tuplekey_create_without_gpu_fails_loudly():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present; covered by -m gpu tests")
    from arroyo_amd import gpu
    lib = gpu.lib()
    cfg = cabi.make_tuplekey_config(2)
    h = lib.arroyo_amd_tuplekey_create(ctypes.byref(cfg))
    assert not h, "create must fail without a HIP device (no CPU fallback)"
    msg = lib.arroyo_amd_tuplekey_last_error(None).decode()
    assert "device" in msg.lower()
    with pytest.raises(RuntimeError, match="(?i)device"):
        gpu.make_tuplekey(cfg)


def test_create_rejects_n_cols_0_and_9_with_its_own_message():
    """Config validation precedes the device: it needs no GPU."""
    from arroyo_amd import gpu
    for n_cols in (0, 9):
        with pytest.raises(RuntimeError, match="n_cols"):
            gpu.make_tuplekey(cabi.make_tuplekey_config(n_cols))
    with pytest.raises(RuntimeError, match="log2_capacity"):
        gpu.make_tuplekey(cabi.make_tuplekey_config(2, log2_capacity=31))
    with pytest.raises(RuntimeError, match="hash_bits"):
        gpu.make_tuplekey(cabi.make_tuplekey_config(2, hash_bits=64))


def test_tuple_hash_np_fixed_example():
    """3 rows, 2 columns, row 1's second component NULL (its word garbage):
    the hash worked out step by step from splitmix64_np."""
    a = np.array([5, -1, 0], dtype=np.int64)
    b = np.array([7, 123456789, 0], dtype=np.int64)
    valid = [None, np.array([True, False, True])]
    got = tuple_hash_np([a, b], valid)
    assert got.dtype == np.uint64 and len(got) == 3

    def sm(x):
        return int(splitmix64_np(np.array([x], dtype=np.uint64))[0])

    u = lambda x: x & (2**64 - 1)
    want = [sm(sm(sm(0) ^ u(5)) ^ u(7)),
            sm(sm(sm(2) ^ u(-1)) ^ 0),      # mask bit 1, word read as 0
            sm(sm(sm(0) ^ 0) ^ 0)]
    assert got.tolist() == want
    assert len(set(want)) == 3
    # valid=None is "nothing NULL"; f64 columns hash by their raw bits
    assert tuple_hash_np([a, b])[0] == want[0]
    f = np.array([0.0, -0.0])
    hf = tuple_hash_np([f])
    assert hf[0] != hf[1]
    assert hf[0] == tuple_hash_np([np.zeros(1, dtype=np.int64)])[0]


def test_python_constants_match_the_header():
    hdr = open(os.path.join(ROOT, "include", "arroyo_amd_types.h")).read()
    defs = dict(re.findall(r"#define\s+(AMD_TKEY_[A-Z_]+)\s+(\d+)", hdr))
    assert set(defs) == {"AMD_TKEY_MAX_COLS", "AMD_TKEY_BLOCK_THREADS",
                         "AMD_TKEY_MAX_BLOCKS"}
    for name, value in defs.items():
        assert getattr(cabi, name) == int(value), name
    assert cabi.TKEY_GRID_ROWS == (cabi.AMD_TKEY_BLOCK_THREADS *
                                   cabi.AMD_TKEY_MAX_BLOCKS)
    # the kernels launch by these constants, not by literals of their own
    src = open(os.path.join(ROOT, "arroyo_amd", "csrc", "tuplekey.hip")).read()
    assert "AMD_TKEY_MAX_BLOCKS" in src and "AMD_TKEY_BLOCK_THREADS" in src


# ---- 2. identity, one batch -------------------------------------------------

def adversarial_tuples(n_cols):
    base = tuple(range(100, 100 + n_cols))
    rows = [base,
            base[:-1] + (base[-1] + 1,),          # differ in the last word
            (base[0] + 1,) + base[1:]]            # ... in the first
    for s in range(1, n_cols):                    # permutations of one set
        rows.append(base[s:] + base[:s])
    if n_cols >= 2:
        rows += [(1, 2) + base[2:], (2, 1) + base[2:]]
    for e in (0, -1, I64_MIN, I64_MAX):
        rows.append((e,) * n_cols)
        for p in range(n_cols):
            rows.append((5,) * p + (e,) + (5,) * (n_cols - p - 1))
    return rows


@gpu_only
@pytest.mark.parametrize("n_cols", [1, 2, 3, 8])
def test_identity_one_batch(n_cols):
    rows = shuffled(adversarial_tuples(n_cols), n_cols)
    cols = columns(rows, n_cols)
    keys = keys_of(cols)
    d = make_dict(n_cols)
    ids = d.encode(cols)
    assert ids.dtype == np.int64
    assert_bijection(keys, ids)
    assert decoded_keys(d, ids) == keys
    assert d.count() == len(set(keys))
    d.close()


def null_mask_rows():
    """Every null mask of a 3-column tuple x two word values, each twice with
    different garbage under the NULLs."""
    cols = [[], [], []]
    valid = [[], [], []]
    for mask in range(8):
        for w in (0, 11):
            for garbage in (0x5A5A5A5A5A5A5A5A, -77):
                for c in range(3):
                    null = (mask >> c) & 1
                    cols[c].append(garbage + c if null else w)
                    valid[c].append(not null)
    return ([np.array(c, dtype=np.int64) for c in cols],
            [np.array(v, dtype=bool) for v in valid])


@gpu_only
def test_identity_every_null_mask_and_garbage_under_nulls():
    cols, valid = null_mask_rows()
    rng = np.random.default_rng(3)
    order = rng.permutation(len(cols[0]))
    cols = [c[order] for c in cols]
    valid = [v[order] for v in valid]
    keys = keys_of(cols, valid)
    d = make_dict(3, nullable=True)
    ids = d.encode(cols, valid)
    assert_bijection(keys, ids)
    # 8 masks x 2 words, but under the all-NULL mask both words are one key
    assert len(set(keys)) == 15 and d.count() == 15
    assert decoded_keys(d, ids) == keys
    d.close()


@gpu_only
def test_null_zero_and_zero_null_and_zero_zero_are_three_keys():
    z = np.zeros(3, dtype=np.int64)
    valid = [np.array([False, True, True]), np.array([True, False, True])]
    d = make_dict(2, nullable=True)
    ids = d.encode([z, z], valid)
    assert len(set(ids.tolist())) == 3 and (ids >= 0).all()
    assert decoded_keys(d, ids) == [(1, (0, 0)), (2, (0, 0)), (0, (0, 0))]
    d.close()


@gpu_only
def test_f64_words_compare_as_raw_bits():
    f = np.array([0.0, -0.0, 1.5, 0.0, float("nan")], dtype=np.float64)
    d = make_dict(1)
    ids = d.encode([f])
    assert ids[0] == ids[3] and len(set(ids.tolist())) == 4
    cols, masks = d.decode(ids)
    assert masks is None
    assert np.array_equal(cols[0], f.view(np.int64))
    d.close()


# ---- 3. seams ---------------------------------------------------------------

SEAM_ROWS = [1, 63, 64, 65, 255, 256, 257, cabi.TKEY_GRID_ROWS + 1]


@gpu_only
@pytest.mark.parametrize("n_rows", SEAM_ROWS)
def test_row_count_seams(n_rows):
    rng = np.random.default_rng(n_rows)
    pool = np.array(random_tuples(rng, 300, 2), dtype=np.int64)
    pick = rng.integers(0, len(pool), size=n_rows)
    cols = [np.ascontiguousarray(pool[pick, c]) for c in range(2)]
    keys = keys_of(cols)
    d = make_dict(2)
    ids, hashes = d.encode(cols, want_hashes=True)
    assert_bijection(keys, ids)
    assert np.array_equal(hashes, tuple_hash_np(cols))
    uniq = np.unique(ids)
    assert d.count() == len(uniq) == len(set(keys))
    # the last rows are the ones a short grid-stride loop would drop
    assert decoded_keys(d, ids[-300:]) == keys[-300:]
    d.close()


@gpu_only
@pytest.mark.parametrize("n_rows", [1, 7, 63, 65, 257, 1003,
                                    cabi.TKEY_GRID_ROWS + 1])
def test_validity_seams_and_padding_bits(n_rows):
    """Row counts that are no multiple of 8 or 64; the host bitmap is exactly
    (n_rows + 7) // 8 bytes, and its bits past n_rows, all ones in one run
    and all zeros in the other, change nothing."""
    assert n_rows % 8 and n_rows % 64
    rng = np.random.default_rng(n_rows + 1)
    a = rng.integers(0, 6, size=n_rows).astype(np.int64)
    b = rng.integers(0, 6, size=n_rows).astype(np.int64)
    va = rng.random(n_rows) < 0.7
    vb = rng.random(n_rows) < 0.7
    keys = keys_of([a, b], [va, vb])

    def packed(mask, pad_ones):
        bm = cabi.pack_validity(mask).copy()
        assert len(bm) == (n_rows + 7) // 8
        keep = (1 << (n_rows % 8)) - 1
        bm[-1] = (bm[-1] & keep) | ((0xFF & ~keep) if pad_ones else 0)
        return bm

    d = make_dict(2, nullable=True)
    ids1 = d.encode([a, b], [packed(va, True), packed(vb, True)])
    ids0 = d.encode([a, b], [packed(va, False), packed(vb, False)])
    assert np.array_equal(ids0, ids1)
    assert_bijection(keys, ids0)
    assert d.count() == len(set(keys))
    tail = slice(max(0, n_rows - 200), n_rows)
    assert decoded_keys(d, ids0[tail]) == keys[tail]
    d.close()


# ---- 4. the same-batch race -------------------------------------------------

@gpu_only
@pytest.mark.parametrize("nullable", [False, True])
def test_same_batch_race(nullable):
    rng = np.random.default_rng(40 + nullable)
    d = make_dict(2, log2_capacity=12, nullable=nullable)

    def batch(tuples, pick):
        a = np.array([tuples[i][0] for i in pick], dtype=np.int64)
        b = np.array([tuples[i][1] for i in pick], dtype=np.int64)
        if not nullable:
            return [a, b], None
        # the second component of every third tuple is NULL, and every row
        # carries its own garbage under it
        vb = np.array([i % 3 != 0 for i in pick])
        b = np.where(vb, b, rng.integers(-10**9, 10**9, size=len(pick)))
        return [a, b.astype(np.int64)], [None, vb]

    three = [(1, 2), (2, 1), (-1, -1)]
    cols, valid = batch(three, rng.integers(0, 3, size=4096))
    keys = keys_of(cols, valid)
    ids = d.encode(cols, valid)
    assert_bijection(keys, ids)
    assert len(set(ids.tolist())) == 3 and d.count() == 3

    twins = [(1000 + i, i % 17) for i in range(2048)]
    pick = rng.permutation(np.repeat(np.arange(2048), 2))
    cols, valid = batch(twins, pick)
    keys = keys_of(cols, valid)
    ids2 = d.encode(cols, valid)
    by_key = assert_bijection(keys, ids2)      # every twin got its twin's id
    assert len(by_key) == 2048 and d.count() == 3 + 2048
    assert not set(ids2.tolist()) & set(ids.tolist())
    assert decoded_keys(d, ids2) == keys
    d.close()


# ---- 5. forced collisions ---------------------------------------------------

@gpu_only
@pytest.mark.parametrize("hash_bits", [1, 4])
def test_forced_collisions_stay_exact(hash_bits):
    rng = np.random.default_rng(50 + hash_bits)
    pool = random_tuples(rng, 300, 3, lo=-4, hi=4)
    rows = [pool[i] for i in rng.permutation(np.repeat(np.arange(300), 3))]
    d = make_dict(3, hash_bits=hash_bits)
    ids, hashes = [], []
    for part in (rows[:300], rows[300:600], rows[600:]):
        i, h = d.encode(columns(part, 3), want_hashes=True)
        ids.append(i)
        hashes.append(h)
    ids, hashes = np.concatenate(ids), np.concatenate(hashes)
    keys = keys_of(columns(rows, 3))
    assert_bijection(keys, ids)
    assert len(set(ids.tolist())) == 300 and d.count() == 300
    assert decoded_keys(d, ids) == keys
    # still the full content hash, whatever the table was told to use of it
    assert np.array_equal(hashes, tuple_hash_np(columns(rows, 3)))
    assert len(set(hashes.tolist())) == 300
    d.close()


# ---- 6. other behaviour -----------------------------------------------------

@gpu_only
def test_ids_are_stable_across_batches():
    rng = np.random.default_rng(6)
    pool = random_tuples(rng, 600, 2)
    pool = [pool[i] for i in rng.permutation(600)]
    d = make_dict(2)
    first = dict(zip(pool[:200], d.encode(columns(pool[:200], 2)).tolist()))
    known = dict(first)
    for new in (pool[200:400], pool[400:600]):
        mixed = pool[:100] + list(known)[150:250] + new
        mixed = [mixed[i] for i in rng.permutation(len(mixed))]
        ids = d.encode(columns(mixed, 2)).tolist()
        assert_bijection(mixed, ids)
        fresh = set()
        for t, i in zip(mixed, ids):
            if t in known:
                assert i == known[t]
            else:
                fresh.add(i)
        assert len(fresh) == 200 and not fresh & set(known.values())
        known.update(zip(mixed, ids))
    assert d.count() == 600
    d.close()


@gpu_only
def test_content_hash_is_handle_independent_and_hash_device_is_stateless():
    import torch
    cols, valid = null_mask_rows()
    want = tuple_hash_np(cols, valid)
    a = make_dict(3, nullable=True, log2_capacity=10, hash_bits=0)
    b = make_dict(3, nullable=True, log2_capacity=12, hash_bits=5)
    _, ha = a.encode(cols, valid, want_hashes=True)
    _, hb = b.encode(cols, valid, want_hashes=True)
    assert ha.dtype == np.uint64
    assert np.array_equal(ha, want) and np.array_equal(hb, want)
    a.close()
    b.close()

    n = len(cols[0])
    c = make_dict(3, nullable=True)
    t_cols = [torch.from_numpy(x).cuda() for x in cols]
    t_bm = [torch.from_numpy(device_bitmap(v)).cuda() for v in valid]
    t_hash = torch.zeros(n, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    c.hash_device([t.data_ptr() for t in t_cols],
                  [t.data_ptr() for t in t_bm], n, t_hash.data_ptr())
    assert np.array_equal(t_hash.cpu().numpy().view(np.uint64), want)
    assert c.count() == 0 and len(c.drain()[0]) == 0
    c.close()


def device_bitmap(mask):
    """An Arrow bitmap padded to whole 64-bit words, as the device surface
    takes it."""
    n = len(mask)
    bm = np.zeros((n + 63) // 64 * 8, dtype=np.uint8)
    bm[:(n + 7) // 8] = cabi.pack_validity(mask)
    return bm


def validity_words(mask, n):
    """What decode_device must write for a column: little-endian 64-bit
    words, bit r = row r non-null, bits past n clear."""
    full = np.ones(n, dtype=bool) if mask is None else mask
    return device_bitmap(full).view(np.uint64)


@gpu_only
def test_device_surface_matches_host_surface():
    import torch
    cols, valid = null_mask_rows()
    cols = [np.tile(c, 15)[:-3] for c in cols]      # 477 rows: no multiple
    valid = [np.tile(v, 15)[:-3] for v in valid]    # of 8 or 64
    valid[2] = np.ones_like(valid[2])               # one column never NULL
    n = len(cols[0])
    d = make_dict(3, nullable=True)
    t_cols = [torch.from_numpy(x).cuda() for x in cols]
    t_bm = [torch.from_numpy(device_bitmap(v)).cuda() for v in valid]
    t_ids = torch.full((n,), -7, dtype=torch.int64, device="cuda")
    t_hash = torch.zeros(n, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    d.encode_device([t.data_ptr() for t in t_cols],
                    [t_bm[0].data_ptr(), t_bm[1].data_ptr(), None], n,
                    t_ids.data_ptr(), t_hash.data_ptr())
    dev_ids = t_ids.cpu().numpy()
    host_ids, host_hashes = d.encode(cols, valid, want_hashes=True)
    assert np.array_equal(dev_ids, host_ids)
    assert np.array_equal(t_hash.cpu().numpy().view(np.uint64), host_hashes)
    assert_bijection(keys_of(cols, valid), dev_ids)

    n_words = (n + 63) // 64
    o_cols = [torch.full((n,), -7, dtype=torch.int64, device="cuda")
              for _ in range(3)]
    o_bm = [torch.full((n_words,), -1, dtype=torch.int64, device="cuda")
            for _ in range(3)]
    torch.cuda.synchronize()
    d.decode_device(t_ids.data_ptr(), n, [t.data_ptr() for t in o_cols],
                    [t.data_ptr() for t in o_bm])
    h_cols, h_masks = d.decode(host_ids)
    assert h_masks is not None and h_masks[2] is None
    for c in range(3):
        assert np.array_equal(o_cols[c].cpu().numpy(), h_cols[c])
        got = o_bm[c].cpu().numpy().view(np.uint64)
        assert np.array_equal(got, validity_words(h_masks[c], n)), c
        assert int(got[-1]) >> (n % 64) == 0, "bits past n_rows are 0"
    d.close()


# ---- 7. decode --------------------------------------------------------------

@gpu_only
def test_decode_validity_only_where_a_null_is():
    a = np.array([1, 2, 3, 4, 5, 6], dtype=np.int64)
    b = np.array([9, 9, 9, 9, 9, 9], dtype=np.int64)
    c = np.array([0, 0, 7, 7, 0, 0], dtype=np.int64)
    valid = [None,
             np.array([True, True, False, False, True, True]),
             np.array([True, True, True, False, True, False])]
    d = make_dict(3, nullable=True)
    ids = d.encode([a, b, c], valid)
    keys = keys_of([a, b, c], valid)
    assert decoded_keys(d, ids) == keys
    # no NULL among the requested ids: no validity at all
    cols, masks = d.decode(ids[[0, 1, 4]])
    assert masks is None
    assert [x.tolist() for x in cols] == [[1, 2, 5], [9, 9, 9], [0, 0, 0]]
    # only column 1 holds a NULL among these
    cols, masks = d.decode(ids[[0, 2, 1]])
    assert masks[0] is None and masks[2] is None
    assert masks[1].tolist() == [True, False, True]
    assert cols[1].tolist() == [9, 0, 9] and cols[2].tolist() == [0, 7, 0]
    # columns 1 and 2, never column 0
    cols, masks = d.decode(ids)
    assert masks[0] is None
    assert masks[1].tolist() == valid[1].tolist()
    assert masks[2].tolist() == valid[2].tolist()
    assert cols[2].tolist() == [0, 0, 7, 0, 0, 0]
    # a non-nullable handle never returns validity
    e = make_dict(2)
    cols, masks = e.decode(e.encode([a, b]))
    assert masks is None and cols[0].tolist() == a.tolist()
    d.close()
    e.close()


# ---- 8. errors --------------------------------------------------------------

@gpu_only
def test_capacity_exhaustion_is_loud_and_keeps_earlier_tuples():
    """16 slots, limit 7/8 = 14: the 15th distinct tuple must fail."""
    rows = [(i, -i) for i in range(15)]
    d = make_dict(2, log2_capacity=4)
    ids = d.encode(columns(rows[:14], 2))
    assert_bijection(rows[:14], ids)
    assert d.count() == 14
    with pytest.raises(RuntimeError, match="capacity"):
        d.encode(columns(rows[14:], 2))
    assert d.count() == 14
    assert decoded_keys(d, ids) == keys_of(columns(rows[:14], 2))
    assert np.array_equal(d.encode(columns(rows[:14], 2)), ids)
    d.close()
    # the same in one call: 15 new tuples do not fit either
    e = make_dict(2, log2_capacity=4)
    with pytest.raises(RuntimeError, match="capacity"):
        e.encode(columns(rows, 2))
    e.close()


@gpu_only
def test_decode_of_an_unissued_id_is_an_error():
    d = make_dict(2)
    d.encode(columns([(1, 2), (2, 1), (3, 3)], 2))
    issued = set(d.drain()[0].tolist())
    assert len(issued) == 3
    unissued = next(i for i in range(1 << 10) if i not in issued)
    for bad in (-1, 1 << 10, unissued):
        with pytest.raises(RuntimeError, match="never issued"):
            d.decode(np.array([min(issued), bad], dtype=np.int64))
    d.close()


@gpu_only
def test_bitmap_on_a_non_nullable_handle_is_an_error():
    a = np.arange(5, dtype=np.int64)
    d = make_dict(2)
    with pytest.raises(RuntimeError, match="nullable"):
        d.encode([a, a], [None, np.ones(5, dtype=bool)])
    assert d.count() == 0
    assert len(d.encode([a, a], [None, None])) == 5   # no bitmap: fine
    d.close()


@gpu_only
def test_n_rows_over_the_limit_is_an_error():
    """The limit is checked before any buffer is touched, so tiny buffers
    will do."""
    a = np.zeros(1, dtype=np.int64)
    ids = np.zeros(1, dtype=np.int64)
    d = make_dict(1)
    assert cabi.TKEY_MAX_ROWS == 2**31 - 2
    rc = d._fn["encode"](d._h, cabi._ptr_array([a.ctypes.data]), None,
                         cabi.TKEY_MAX_ROWS + 1, ids.ctypes.data, None)
    assert rc != 0
    assert "limit" in d._fn["last_error"](d._h).decode()
    assert d.count() == 0
    d.close()


@gpu_only
def test_zero_rows():
    d = make_dict(2, nullable=True)
    e = np.zeros(0, dtype=np.int64)
    ids = d.encode([e, e], [None, np.zeros(0, dtype=bool)])
    assert ids.dtype == np.int64 and len(ids) == 0
    cols, masks = d.decode(e)
    assert len(cols) == 2 and all(len(c) == 0 for c in cols) and masks is None
    ids, cols, masks = d.drain()
    assert len(ids) == 0 and len(cols) == 2 and masks is None
    d.restore(e, [e, e])
    d.encode_device([None, None], None, 0, None)
    d.decode_device(None, 0, [None, None], [None, None])
    assert d.count() == 0
    d.close()


@gpu_only
def test_restore_into_a_non_empty_handle_is_an_error():
    d = make_dict(2)
    d.encode(columns([(1, 2), (2, 1)], 2))
    ids, cols, masks = d.drain()
    e = make_dict(2)
    e.encode(columns([(5, 5)], 2))
    with pytest.raises(RuntimeError, match="non-empty"):
        e.restore(ids, cols, masks)
    assert e.count() == 1
    d.close()
    e.close()


@gpu_only
def test_restore_into_a_mismatched_handle_is_an_error():
    rng = np.random.default_rng(8)
    cols, valid = null_mask_rows()
    extra = columns(random_tuples(rng, 200, 3), 3)
    d = make_dict(3, nullable=True, log2_capacity=10, hash_bits=0)
    d.encode(cols, valid)
    d.encode(extra)
    ids, dcols, masks = d.drain()
    d.close()
    assert masks is not None and 200 <= len(ids) <= 215

    def expect_error(match, n_cols=3, **kw):
        kw.setdefault("nullable", True)
        e = make_dict(n_cols, **kw)
        with pytest.raises((RuntimeError, ValueError), match=match):
            e.restore(ids, dcols, masks)
        assert e.count() == 0   # a failed restore leaves the handle empty
        assert len(e.drain()[0]) == 0
        e.close()

    expect_error("log2_capacity", log2_capacity=12)
    expect_error("log2_capacity", log2_capacity=7)
    expect_error("hash_bits", hash_bits=3)
    expect_error("nullable", nullable=False)
    expect_error("columns", n_cols=2)


# ---- 9. checkpoint round trip -----------------------------------------------

@gpu_only
def test_checkpoint_round_trip_keeps_ids():
    rng = np.random.default_rng(9)
    pool = random_tuples(rng, 750, 3)
    pool = [pool[i] for i in rng.permutation(750)]
    old, new = pool[:500], pool[500:]

    def batch(tuples):
        """every fifth tuple's middle component is NULL"""
        cols = columns(tuples, 3)
        valid = [None, np.array([hash(t) % 5 != 0 for t in tuples]), None]
        return cols, valid

    d = make_dict(3, nullable=True, log2_capacity=11)
    cols, valid = batch(old)
    old_keys = keys_of(cols, valid)
    assert any(k[0] for k in old_keys), "NULL-bearing tuples are in"
    drained_want = dict(zip(old_keys, d.encode(cols, valid).tolist()))
    ids, dcols, masks = d.drain()
    d.close()
    assert masks is not None and masks[0] is None and masks[2] is None
    drained = dict(zip(keys_of(dcols, masks), ids.tolist()))
    assert drained == drained_want

    e = make_dict(3, nullable=True, log2_capacity=11)
    e.restore(ids, dcols, masks)
    assert e.count() == len(drained)
    mixed = old[:250] + new
    mixed = [mixed[i] for i in rng.permutation(len(mixed))]
    cols, valid = batch(mixed)
    keys = keys_of(cols, valid)
    got = e.encode(cols, valid)
    assert_bijection(keys, got)
    fresh = set()
    for k, i in zip(keys, got.tolist()):
        if k in drained:
            assert i == drained[k]
        else:
            fresh.add(i)
    assert not fresh & set(drained.values())
    assert e.count() == len(drained) + len(fresh)
    assert decoded_keys(e, got) == keys
    e.close()
