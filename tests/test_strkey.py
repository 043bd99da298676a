"""Device string-key dictionary (arroyo_amd_strkey_*): an interner for Arrow
Utf8 key columns.  The checker throughout is a Python dict / set: equal byte
strings must get equal ids, different byte strings different ids, and decode
must give the bytes back.  Ids are opaque; nothing here assumes their values
or density, only id >= 0."""
import ctypes

import numpy as np
import pytest

from arroyo_amd import cabi
from arroyo_amd.cabi import arrow_to_strings, strings_to_arrow

gpu_only = pytest.mark.gpu


def make_dict(**kw):
    from arroyo_amd import gpu
    kw.setdefault("log2_capacity", 10)
    kw.setdefault("arena_bytes", 1 << 20)
    return gpu.make_strkey(cabi.make_strkey_config(**kw))


def adversarial_strings():
    base64 = bytes(range(1, 64))
    strs = [b"", b"a", b"a\x00", b"\x00", b"ab", b"abc",
            base64 + b"x", base64 + b"y",            # differ in the last byte
            b"Xcommon-suffix-0123", b"Ycommon-suffix-0123"]   # ... the first
    strs += [b"\xff" * n
             for n in (0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 255, 1000)]
    return strs


def random_strings(rng, n, max_len):
    """n distinct random byte strings of length 0..max_len."""
    seen = set()
    while len(seen) < n:
        ln = int(rng.integers(0, max_len + 1))
        seen.add(rng.integers(0, 256, size=ln, dtype=np.uint8).tobytes())
    return sorted(seen)


def assert_bijection(strings, ids):
    """ids[i] == ids[j] iff strings[i] == strings[j], and every id >= 0."""
    assert len(strings) == len(ids)
    assert (np.asarray(ids) >= 0).all()
    by_str, by_id = {}, {}
    for s, i in zip(strings, ids):
        i = int(i)
        assert by_str.setdefault(s, i) == i, f"{s!r} got two ids"
        assert by_id.setdefault(i, s) == s, \
            f"id {i} given to {by_id[i]!r} and {s!r}"


# ---- 1. CPU ---------------------------------------------------------------

def test_strkey_create_without_gpu_fails_loudly():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present; covered by -m gpu tests")
    from arroyo_amd import gpu
    lib = gpu.lib()
    cfg = cabi.make_strkey_config()
    h = lib.arroyo_amd_strkey_create(ctypes.byref(cfg))
    assert not h, "create must fail without a HIP device (no CPU fallback)"
    msg = lib.arroyo_amd_strkey_last_error(None).decode()
    assert "device" in msg.lower()
    with pytest.raises(RuntimeError, match="(?i)device"):
        gpu.make_strkey(cfg)


def test_strings_to_arrow_round_trip():
    strs = adversarial_strings() + ["héllo", "plain"]
    offsets, data = strings_to_arrow(strs)
    assert offsets.dtype == np.int32 and data.dtype == np.uint8
    assert offsets[0] == 0 and len(offsets) == len(strs) + 1
    assert offsets[-1] == len(data)
    want = [s.encode("utf-8") if isinstance(s, str) else s for s in strs]
    assert arrow_to_strings(offsets, data) == want
    # a sliced array: offsets[0] != 0
    sliced = arrow_to_strings(offsets[3:] + 13,
                              np.concatenate([np.zeros(13, np.uint8), data]))
    assert sliced == want[3:]
    o0, d0 = strings_to_arrow([])
    assert list(o0) == [0] and len(d0) == 0 and arrow_to_strings(o0, d0) == []


# ---- 2. byte-exact identity, one batch ------------------------------------

def shuffled_adversarial(seed):
    rng = np.random.default_rng(seed)
    strs = adversarial_strings() * 3
    return [strs[i] for i in rng.permutation(len(strs))]


@gpu_only
def test_byte_exact_identity_one_batch():
    strs = shuffled_adversarial(1)
    d = make_dict()
    ids = d.encode(*strings_to_arrow(strs))
    assert_bijection(strs, ids)
    assert arrow_to_strings(*d.decode(ids)) == strs
    assert d.count() == len(set(strs))
    d.close()


# ---- 3. sliced input ------------------------------------------------------

@gpu_only
def test_sliced_input_gets_the_same_ids():
    strs = shuffled_adversarial(2)
    offsets, data = strings_to_arrow(strs)
    junk = np.arange(200, 213, dtype=np.uint8)
    d = make_dict()
    ids_sliced = d.encode(offsets + 13, np.concatenate([junk, data]))
    ids_plain = d.encode(offsets, data)
    assert np.array_equal(ids_sliced, ids_plain)
    assert_bijection(strs, ids_plain)
    assert d.count() == len(set(strs))
    d.close()


# ---- 4. the same-batch race -----------------------------------------------

@gpu_only
def test_same_batch_race():
    d = make_dict()
    n = 65536
    ids = d.encode(*strings_to_arrow([b"hello-world"] * n))
    assert len(ids) == n and ids[0] >= 0
    assert (ids == ids[0]).all()
    assert d.count() == 1
    rng = np.random.default_rng(4)
    pool = [b"alpha", b"beta-beta", b""]
    strs = [pool[i] for i in rng.integers(0, 3, size=4096)]
    ids2 = d.encode(*strings_to_arrow(strs))
    assert_bijection(strs, ids2)
    assert len(set(ids2.tolist())) == 3
    assert int(ids[0]) not in set(ids2.tolist())
    assert d.count() == 4
    d.close()


# ---- 5. forced collisions -------------------------------------------------

@gpu_only
def test_forced_collisions_stay_exact():
    rng = np.random.default_rng(5)
    pool = random_strings(rng, 300, 24)
    rows = [pool[i] for i in rng.permutation(np.repeat(np.arange(300), 4))]
    d = make_dict(hash_bits=2)
    all_ids, all_hashes = [], []
    for part in (rows[:400], rows[400:800], rows[800:]):
        ids, hashes = d.encode(*strings_to_arrow(part), with_hashes=True)
        all_ids.append(ids)
        all_hashes.append(hashes)
    ids = np.concatenate(all_ids)
    hashes = np.concatenate(all_hashes)
    assert_bijection(rows, ids)
    assert len(set(ids.tolist())) == 300 and d.count() == 300
    assert arrow_to_strings(*d.decode(ids)) == rows
    by_str = {}
    for s, h in zip(rows, hashes):
        assert by_str.setdefault(s, int(h)) == int(h)
    d.close()


# ---- 6. stability across batches ------------------------------------------

@gpu_only
def test_ids_are_stable_across_batches():
    rng = np.random.default_rng(6)
    pool = random_strings(rng, 400, 30)
    old, new = pool[:200], pool[200:]
    d = make_dict()
    first = dict(zip(old, d.encode(*strings_to_arrow(old)).tolist()))
    mixed = old[:100] + new[:100]
    mixed = [mixed[i] for i in rng.permutation(len(mixed))]
    ids = d.encode(*strings_to_arrow(mixed)).tolist()
    assert_bijection(mixed, ids)
    new_ids = set()
    for s, i in zip(mixed, ids):
        if s in first:
            assert i == first[s]
        else:
            new_ids.add(i)
    assert len(new_ids) == 100
    assert not new_ids & set(first.values())
    assert d.count() == 300
    d.close()


# ---- 7. the content hash is handle-independent ----------------------------

@gpu_only
def test_content_hash_is_handle_independent():
    rng = np.random.default_rng(7)
    pool = random_strings(rng, 300, 24)
    arrow = strings_to_arrow(pool)
    a = make_dict(hash_bits=0)
    b = make_dict(hash_bits=5)
    _, ha = a.encode(*arrow, with_hashes=True)
    _, hb = b.encode(*arrow, with_hashes=True)
    a.close()
    b.close()
    assert ha.dtype == np.uint64
    assert np.array_equal(ha, hb)
    assert len(set(ha.tolist())) >= 290


# ---- 8. device surface ----------------------------------------------------

@gpu_only
def test_device_surface_matches_host_surface():
    import torch
    strs = shuffled_adversarial(8)
    offsets, data = strings_to_arrow(strs)
    d = make_dict()
    t_off = torch.from_numpy(offsets).cuda()
    t_data = torch.from_numpy(data).cuda()
    t_ids = torch.full((len(strs),), -7, dtype=torch.int64, device="cuda")
    t_hash = torch.zeros(len(strs), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    d.encode_device(t_off.data_ptr(), t_data.data_ptr(), len(strs),
                    t_ids.data_ptr(), t_hash.data_ptr())
    dev_ids = t_ids.cpu().numpy()
    host_ids, host_hashes = d.encode(offsets, data, with_hashes=True)
    assert np.array_equal(dev_ids, host_ids)
    assert np.array_equal(t_hash.cpu().numpy().view(np.uint64), host_hashes)
    assert_bijection(strs, dev_ids)
    d.close()


@gpu_only
def test_lookup_kernel_timing_is_opt_in():
    strs = [b"k%04d" % i for i in range(2000)]
    arrow = strings_to_arrow(strs)
    d = make_dict(log2_capacity=12)
    ids = d.encode(*arrow)
    assert d.profile() == 0.0            # off by default: nothing timed
    d.profile(True)
    assert np.array_equal(d.encode(*arrow), ids)
    ms = d.profile()
    assert 0.0 < ms < 1000.0
    d.profile(False)
    assert np.array_equal(d.encode(*arrow), ids)
    assert d.profile() == ms             # the last timed encode stays
    d.close()


# ---- 9. errors ------------------------------------------------------------

@gpu_only
def test_decreasing_offsets_are_an_error():
    d = make_dict()
    with pytest.raises(RuntimeError, match="offsets"):
        d.encode(np.array([0, 5, 3, 8], dtype=np.int32),
                 np.zeros(8, dtype=np.uint8))
    assert d.count() == 0
    d.close()


@gpu_only
def test_capacity_exhaustion_is_loud_and_keeps_earlier_strings():
    strs = [b"key-%02d" % i for i in range(17)]
    d = make_dict(log2_capacity=4)
    ids = d.encode(*strings_to_arrow(strs[:8]))
    assert_bijection(strs[:8], ids)
    with pytest.raises(RuntimeError, match="capacity"):
        d.encode(*strings_to_arrow(strs[8:]))
    assert arrow_to_strings(*d.decode(ids)) == strs[:8]
    d.close()


@gpu_only
def test_arena_exhaustion_is_loud_and_keeps_earlier_strings():
    strs = [bytes([65 + i]) * 100 for i in range(4)]
    d = make_dict(arena_bytes=256)
    ids = d.encode(*strings_to_arrow(strs[:2]))
    assert_bijection(strs[:2], ids)
    with pytest.raises(RuntimeError, match="arena"):
        d.encode(*strings_to_arrow(strs[2:]))
    assert arrow_to_strings(*d.decode(ids)) == strs[:2]
    d.close()


@gpu_only
def test_decode_of_an_unissued_id_is_an_error():
    d = make_dict()
    d.encode(*strings_to_arrow([b"one", b"two", b"three"]))
    issued = set(d.drain()[0].tolist())
    assert len(issued) == 3
    unissued = next(i for i in range(1 << 10) if i not in issued)
    with pytest.raises(RuntimeError):
        d.decode(np.array([unissued], dtype=np.int64))
    with pytest.raises(RuntimeError):
        d.decode(np.array([-1], dtype=np.int64))
    with pytest.raises(RuntimeError):
        d.decode(np.array([1 << 40], dtype=np.int64))
    d.close()


@gpu_only
def test_restore_into_a_non_empty_handle_is_an_error():
    d = make_dict()
    d.encode(*strings_to_arrow([b"one", b"two"]))
    ids, offsets, data = d.drain()
    e = make_dict()
    e.encode(*strings_to_arrow([b"occupied"]))
    with pytest.raises(RuntimeError, match="non-empty"):
        e.restore(ids, offsets, data)
    d.close()
    e.close()


@gpu_only
def test_zero_rows():
    d = make_dict()
    empty_off = np.zeros(1, dtype=np.int32)
    empty_data = np.zeros(0, dtype=np.uint8)
    ids = d.encode(empty_off, empty_data)
    assert ids.dtype == np.int64 and len(ids) == 0
    offsets, data = d.decode(np.zeros(0, dtype=np.int64))
    assert list(offsets) == [0] and len(data) == 0
    ids, offsets, data = d.drain()
    assert len(ids) == 0 and list(offsets) == [0] and len(data) == 0
    assert d.count() == 0
    d.close()


# ---- 10. checkpoint round trip --------------------------------------------

@gpu_only
def test_checkpoint_round_trip_keeps_ids():
    rng = np.random.default_rng(10)
    pool = random_strings(rng, 750, 32)
    pool = [pool[i] for i in rng.permutation(len(pool))]
    old, new = pool[:500], pool[500:]
    d = make_dict(log2_capacity=11)
    d.encode(*strings_to_arrow(old))
    ids, offsets, data = d.drain()
    d.close()
    drained = dict(zip(arrow_to_strings(offsets, data), ids.tolist()))
    assert set(drained) == set(old) and len(set(drained.values())) == 500

    e = make_dict(log2_capacity=11)
    e.restore(ids, offsets, data)
    assert e.count() == 500
    mixed = old[:250] + new
    mixed = [mixed[i] for i in rng.permutation(len(mixed))]
    got = e.encode(*strings_to_arrow(mixed)).tolist()
    assert_bijection(mixed, got)
    new_ids = set()
    for s, i in zip(mixed, got):
        if s in drained:
            assert i == drained[s]
        else:
            new_ids.add(i)
    assert len(new_ids) == 250
    assert not new_ids & set(drained.values())
    assert e.count() == 750
    assert arrow_to_strings(*e.decode(np.array(got, dtype=np.int64))) == mixed
    e.close()


@gpu_only
def test_restore_with_another_capacity_is_an_error():
    d = make_dict(log2_capacity=10)
    d.encode(*strings_to_arrow([b"k%03d" % i for i in range(200)]))
    ids, offsets, data = d.drain()
    d.close()
    e = make_dict(log2_capacity=12)
    with pytest.raises(RuntimeError, match="log2_capacity"):
        e.restore(ids, offsets, data)
    assert e.count() == 0   # a failed restore leaves the handle empty
    e.close()
