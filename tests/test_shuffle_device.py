"""Stable device partition for the keyed shuffle (arroyo_amd_shuffle_*):
exact, bit-for-bit equality with the host restatement
(shuffle.partition_host: device owner rule + stable argsort), for fixed-width
columns and for an Arrow Utf8 column riding along."""
import numpy as np
import pytest

from arroyo_amd import cabi
from arroyo_amd.cabi import arrow_to_strings, strings_to_arrow
from arroyo_amd.shuffle import KEY_HASH, KEY_I64, partition_host

pytestmark = pytest.mark.gpu

TILE = cabi.AMD_SHUF_TILE_ROWS
M64 = (1 << 64) - 1
SIZES = (0, 1, 63, 64, 65, 255, 256, 257, TILE - 1, TILE, TILE + 1, 20_011)
MAX_ROWS = 20_480


def dev():
    import torch
    return torch.device("cuda", 0)


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def make(n_parts, n_cols, key_col=0, key_mode=KEY_I64, has_utf8=False,
         max_rows=MAX_ROWS, max_bytes=0):
    from arroyo_amd import gpu
    return gpu.make_shuffler(cabi.make_shuffle_config(
        n_parts, n_cols, key_col=key_col, key_mode=key_mode,
        has_utf8=has_utf8, max_rows=max_rows, max_bytes=max_bytes))


def run_and_check(sh, cols, utf8=None, rowid_col=None):
    """One device call checked against the host restatement.  cols: numpy
    8-byte columns; utf8: (offsets, data) numpy or None.  Returns the device
    result as host arrays (cols, row_start, offsets, data, byte_start)."""
    cfg = sh.cfg
    want = partition_host(cols, cfg.key_col, cfg.key_mode, cfg.n_parts, utf8)
    got = sh.partition([to_dev(c) for c in cols],
                       None if utf8 is None else (to_dev(utf8[0]),
                                                  to_dev(utf8[1])))
    assert got.row_start == want.row_start
    gcols = [c.cpu().numpy() for c in got.cols]
    for g, w in zip(gcols, want.cols):
        assert g.dtype == w.dtype
        assert np.array_equal(g.view(np.int64), w.view(np.int64))
    if rowid_col is not None:
        # stable, independently of the restatement: input row numbers are
        # strictly increasing inside every partition
        rows = gcols[rowid_col]
        for p in range(cfg.n_parts):
            seg = rows[got.row_start[p]:got.row_start[p + 1]]
            assert (np.diff(seg) > 0).all()
    goff = gdata = None
    if utf8 is not None:
        assert got.byte_start == want.byte_start
        goff = got.utf8_offsets.cpu().numpy()
        gdata = got.utf8_data.cpu().numpy()
        assert np.array_equal(goff, want.utf8_offsets)
        assert np.array_equal(gdata, want.utf8_data)
    return gcols, got.row_start, goff, gdata, got.byte_start


def columns(rng, n, n_cols, key_col, keys):
    """n_cols columns: the key where asked, the input row number in the
    first free column, then random planes (one of them f64 bit patterns)."""
    cols = [None] * n_cols
    cols[key_col] = np.asarray(keys)
    rowid_col = None
    for c in range(n_cols):
        if cols[c] is not None:
            continue
        if rowid_col is None:
            rowid_col = c
            cols[c] = np.arange(n, dtype=np.int64)
        elif c % 3 == 2:
            cols[c] = rng.random(n)
        else:
            cols[c] = rng.integers(-2**62, 2**62, size=n).astype(np.int64)
    return cols, rowid_col


@pytest.mark.parametrize("n_parts", [1, 2, 3, 8, 64])
def test_fixed_width_matches_host_exactly(n_parts):
    rng = np.random.default_rng(1000 + n_parts)
    keysets = {}
    for n in SIZES:
        keysets[n] = (rng.integers(-10**6, 10**6, size=n).astype(np.int64),
                      rng.integers(0, 1 << 63, size=n, dtype=np.uint64) * 2
                      + rng.integers(0, 2, size=n, dtype=np.uint64))
    for n_cols, key_col in ((1, 0), (3, 0), (3, 2), (16, 0), (16, 15)):
        for key_mode in (KEY_I64, KEY_HASH):
            sh = make(n_parts, n_cols, key_col, key_mode)
            for n in SIZES:
                cols, rid = columns(rng, n, n_cols, key_col,
                                    keysets[n][key_mode])
                run_and_check(sh, cols, rowid_col=rid)
            sh.close()


def hashes_for_owners(owners, n_parts):
    """KEY_HASH keys whose device owner is exactly owners[i]."""
    owners = np.asarray(owners, dtype=np.uint64)
    if n_parts == 1:
        return np.arange(len(owners), dtype=np.uint64)
    rng_size = np.uint64(M64 // n_parts + 1)
    return owners * rng_size + np.arange(len(owners), dtype=np.uint64) % \
        np.uint64(1000)


@pytest.mark.parametrize("n_parts", [1, 3, 8, 64])
def test_key_distributions(n_parts):
    rng = np.random.default_rng(2000 + n_parts)
    n = 3 * TILE + 77
    r = np.arange(n)
    sh_i = make(n_parts, 3, 0, KEY_I64)
    sh_h = make(n_parts, 3, 0, KEY_HASH)
    # every row one key: one partition takes everything
    cols, rid = columns(rng, n, 3, 0, np.full(n, 42, dtype=np.int64))
    _, row_start, *_ = run_and_check(sh_i, cols, rowid_col=rid)
    assert sorted(np.diff(row_start))[-1] == n
    # every wave holds a single owner
    cols, rid = columns(rng, n, 3, 0,
                        hashes_for_owners((r // 64) % n_parts, n_parts))
    run_and_check(sh_h, cols, rowid_col=rid)
    # every lane of a wave has a different owner (as far as n_parts allows)
    cols, rid = columns(rng, n, 3, 0, hashes_for_owners(r % n_parts, n_parts))
    _, row_start, *_ = run_and_check(sh_h, cols, rowid_col=rid)
    assert min(np.diff(row_start)) >= n // n_parts
    # the highest owner, up to the last hash
    cols, rid = columns(rng, n, 3, 0, np.uint64(M64) - r.astype(np.uint64))
    _, row_start, *_ = run_and_check(sh_h, cols, rowid_col=rid)
    assert row_start[n_parts - 1] == 0 or n_parts == 1
    # a Zipf draw
    cols, rid = columns(rng, n, 3, 0,
                        (rng.zipf(1.2, size=n) % 5000).astype(np.int64))
    run_and_check(sh_i, cols, rowid_col=rid)
    sh_i.close()
    sh_h.close()


def test_two_calls_are_byte_identical():
    rng = np.random.default_rng(3)
    n = 20_011
    keys = (rng.zipf(1.3, size=n) % 300).astype(np.int64)
    strs = [b"k%d" % k * (1 + k % 3) for k in keys]
    utf8 = strings_to_arrow(strs)
    sh = make(8, 3, 1, KEY_I64, has_utf8=True, max_bytes=len(utf8[1]))
    cols, rid = columns(rng, n, 3, 1, keys)
    a = run_and_check(sh, cols, utf8, rowid_col=rid)
    b = run_and_check(sh, cols, utf8, rowid_col=rid)
    for x, y in zip(a[0], b[0]):
        assert x.tobytes() == y.tobytes()
    assert a[1] == b[1] and a[4] == b[4]
    assert a[2].tobytes() == b[2].tobytes()
    assert a[3].tobytes() == b[3].tobytes()
    sh.close()


def edge_strings(rng, n):
    """Lengths around the 8-byte word and the wave-copy threshold, one of
    several KB, embedded NUL, bytes >= 0x80, and random filler."""
    fixed = [rng.integers(0, 256, size=ln, dtype=np.uint8).tobytes()
             for ln in (0, 1, 7, 8, 9, 31, 32, 33, 63, 64, 65, 511, 512, 513,
                        5003)]
    fixed += [b"a\x00b\x00", b"\x00", b"\xff\xfe\x80caf\xc3\xa9", b""]
    out = []
    for i in range(n):
        if i % 37 < len(fixed) and i < 37 * 3:
            out.append(fixed[i % 37])
        else:
            ln = int(rng.integers(0, 24))
            out.append(rng.integers(0, 256, size=ln, dtype=np.uint8)
                       .tobytes())
    return out


def check_segments(strs, cols_out, rid, row_start, off, data, byte_start,
                   n_parts):
    """Every partition is a standalone Utf8 array holding its rows' strings."""
    for p in range(n_parts):
        lo, hi = row_start[p], row_start[p + 1]
        o = off[lo + p:hi + p + 1]
        d = data[byte_start[p]:byte_start[p + 1]]
        assert o[0] == 0 and o[-1] == len(d)
        rows = cols_out[rid][lo:hi].tolist()
        assert arrow_to_strings(o, d) == [strs[r] for r in rows]


@pytest.mark.parametrize("n_parts", [1, 3, 8, 64])
def test_utf8_column_rides_along(n_parts):
    rng = np.random.default_rng(4000 + n_parts)
    n = 2 * TILE + 301
    strs = edge_strings(rng, n)
    off, data = strings_to_arrow(strs)
    # a slice of a larger array: offsets[0] != 0, poison around the slice
    POISON = 0xA5
    clean = [s.replace(bytes([POISON]), b"\x5a") for s in strs]
    off, data = strings_to_arrow(clean)
    lead, tail = 13, 4099
    off2 = (off.astype(np.int64) + lead).astype(np.int32)
    data2 = np.concatenate([np.full(lead, POISON, np.uint8), data,
                            np.full(tail, POISON, np.uint8)])
    keys = rng.integers(0, 1 << 63, size=n, dtype=np.uint64) * 2
    sh = make(n_parts, 2, 0, KEY_HASH, has_utf8=True, max_bytes=len(data))
    cols, rid = columns(rng, n, 2, 0, keys)
    gcols, row_start, goff, gdata, byte_start = run_and_check(
        sh, cols, (off2, data2), rowid_col=rid)
    assert byte_start[0] == 0 and byte_start[-1] == len(data)
    assert POISON not in gdata
    check_segments(clean, gcols, rid, row_start, goff, gdata, byte_start,
                   n_parts)
    # only empty strings: every offset 0, no byte moved, data may be empty
    zeros = np.full(n + 1, 7, dtype=np.int32)
    gcols, row_start, goff, gdata, byte_start = run_and_check(
        sh, cols, (zeros, data2[:8]), rowid_col=rid)
    assert not goff.any() and len(gdata) == 0 and not any(byte_start)
    # no rows at all
    e = [c[:0] for c in cols]
    _, row_start, goff, gdata, byte_start = run_and_check(
        sh, e, (np.zeros(1, np.int32), data2[:8]))
    assert not any(row_start) and not any(byte_start) and not goff.any()
    sh.close()


@pytest.mark.parametrize("threshold", [0, 2**31 - 1])
def test_utf8_copy_schemes_agree(threshold):
    """The byte copy has a lane-per-string and a wave-per-string path; each
    alone must move every string."""
    rng = np.random.default_rng(5)
    n = TILE + 9
    strs = edge_strings(rng, n)
    utf8 = strings_to_arrow(strs)
    sh = make(3, 2, 1, KEY_I64, has_utf8=True, max_bytes=len(utf8[1]))
    sh.profile(copy_threshold=threshold)
    cols, rid = columns(rng, n, 2, 1,
                        rng.integers(0, 100, size=n).astype(np.int64))
    gcols, row_start, goff, gdata, byte_start = run_and_check(
        sh, cols, utf8, rowid_col=rid)
    check_segments(strs, gcols, rid, row_start, goff, gdata, byte_start, 3)
    sh.close()


def test_errors_are_loud_and_the_handle_survives():
    import torch
    from arroyo_amd import gpu
    rng = np.random.default_rng(6)
    n = 500
    strs = [b"s%d" % i * (i % 5) for i in range(n)]
    off, data = strings_to_arrow(strs)
    sh = make(3, 2, 0, KEY_I64, has_utf8=True, max_rows=n,
              max_bytes=len(data))
    cols, rid = columns(rng, n, 2, 0,
                        rng.integers(0, 50, size=n).astype(np.int64))

    def good():
        gcols, row_start, goff, gdata, byte_start = run_and_check(
            sh, cols, (off, data), rowid_col=rid)
        check_segments(strs, gcols, rid, row_start, goff, gdata, byte_start, 3)

    def bad(match, cols_, utf8_):
        with pytest.raises(RuntimeError, match=match) as ei:
            sh.partition([to_dev(c) for c in cols_],
                         (to_dev(utf8_[0]), to_dev(utf8_[1])))
        assert str(ei.value)
        good()

    good()
    # one row too many
    big = [np.append(c, c[:1]) for c in cols]
    bad("max_rows", big, (np.append(off, off[-1:]), data))
    # bytes above max_bytes (valid offsets, the bytes really exist)
    fat = np.concatenate([off[:-1], [off[-1] + 1]]).astype(np.int32)
    bad("max_bytes", cols, (fat, np.append(data, np.uint8(1))))
    # malformed offsets, with a data buffer far too small for them: the
    # validation runs on device before any byte is read
    dec = off.copy()
    dec[250] = dec[249] - 1 if dec[249] > 0 else dec[251] + 1
    assert (np.diff(dec.astype(np.int64)) < 0).any()
    bad("offsets", cols, (dec, data[:8]))
    neg = off.copy()
    neg[0] = -5
    bad("offsets", cols, (neg, data[:8]))
    # NULL pointers
    tcols = [to_dev(c) for c in cols]
    toff, tdata = to_dev(off), to_dev(data)
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="NULL"):
        sh.partition_ptrs([tcols[0].data_ptr(), None], n, toff.data_ptr(),
                          tdata.data_ptr())
    good()
    for o_, d_ in ((None, tdata.data_ptr()), (toff.data_ptr(), None),
                   (None, None)):
        with pytest.raises(RuntimeError, match="has_utf8"):
            sh.partition_ptrs([t.data_ptr() for t in tcols], n, o_, d_)
    good()
    sh.close()
    # rejected at create
    for kw in (dict(n_parts=0, n_cols=1), dict(n_parts=65, n_cols=1),
               dict(n_parts=2, n_cols=0), dict(n_parts=2, n_cols=17),
               dict(n_parts=2, n_cols=2, key_col=2),
               dict(n_parts=2, n_cols=2, key_mode=7),
               dict(n_parts=2, n_cols=2, max_rows=0)):
        with pytest.raises(RuntimeError, match="invalid shuffle config"):
            gpu.make_shuffler(cabi.make_shuffle_config(**kw),
                              bind_output=False)


def test_one_handle_many_calls():
    """50 calls of varying sizes on one handle: no scratch of an earlier
    call may leak into a later one."""
    rng = np.random.default_rng(7)
    pool = [rng.integers(0, 256, size=int(ln), dtype=np.uint8).tobytes()
            for ln in rng.integers(0, 70, size=400)]
    sh = make(5, 3, 1, KEY_I64, has_utf8=True, max_rows=6000,
              max_bytes=6000 * 70)
    sizes = [6000, 1, 0, 5999, 64, TILE + 1] + \
        [int(x) for x in rng.integers(0, 6001, size=44)]
    for n in sizes:
        keys = rng.integers(0, 1 + n // 3, size=n).astype(np.int64)
        strs = [pool[i] for i in rng.integers(0, len(pool), size=n)]
        cols, rid = columns(rng, n, 3, 1, keys)
        gcols, row_start, goff, gdata, byte_start = run_and_check(
            sh, cols, strings_to_arrow(strs), rowid_col=rid)
        check_segments(strs, gcols, rid, row_start, goff, gdata, byte_start,
                       5)
    sh.close()
