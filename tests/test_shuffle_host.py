"""Host restatement of the stable keyed shuffle (shuffle.partition_host) and
the exchange built on it (shuffle.shuffle_batch over gloo).  The restatement
is the checker for the device kernels (test_shuffle_device.py), so it is
pinned here against scalar Python; all but the one gpu-marked test run on the
CPU."""
import os
from collections import Counter

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

from arroyo_amd.cabi import arrow_to_strings, strings_to_arrow
from arroyo_amd.shuffle import (KEY_HASH, KEY_I64, owners_device_rule,
                                partition_host, shuffle_batch)

M64 = (1 << 64) - 1


def splitmix64_py(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def owner_py(h, n_parts):
    """The device rule, in Python integers."""
    if n_parts == 1:
        return 0
    return h // (M64 // n_parts + 1)


def test_owner_rule_matches_scalar_restatement():
    rng = np.random.default_rng(5)
    for n_parts in (1, 2, 3, 5, 8, 64):
        edges = [0, 1, M64, M64 - 1, 1 << 63, (1 << 63) - 1]
        rng_size = M64 // n_parts + 1
        for p in range(1, n_parts):        # both sides of every boundary
            edges += [p * rng_size - 1, p * rng_size]
        hs = edges + [int(x) for x in
                      rng.integers(0, 1 << 63, size=200, dtype=np.uint64) * 2]
        got = owners_device_rule(np.array(hs, dtype=np.uint64), n_parts)
        want = [owner_py(h, n_parts) for h in hs]
        assert got.tolist() == want
        assert 0 <= min(want) and max(want) < n_parts
        assert owner_py(0, n_parts) == 0
        assert owner_py(M64, n_parts) == n_parts - 1


def test_key_modes_hash_or_take_the_key_column():
    keys = np.array([0, 1, -1, 12345, -(1 << 63), (1 << 63) - 1],
                    dtype=np.int64)
    for n_parts in (2, 3, 5):
        p = partition_host([keys, np.arange(6)], 0, KEY_I64, n_parts)
        want = [owner_py(splitmix64_py(int(k) & M64), n_parts) for k in keys]
        for q in range(n_parts):
            rows = p.part_cols(q)[1].tolist()
            assert rows == [i for i in range(6) if want[i] == q]
        p = partition_host([keys, np.arange(6)], 0, KEY_HASH, n_parts)
        want = [owner_py(int(k) & M64, n_parts) for k in keys]
        for q in range(n_parts):
            rows = p.part_cols(q)[1].tolist()
            assert rows == [i for i in range(6) if want[i] == q]


def test_partition_is_a_stable_permutation():
    rng = np.random.default_rng(6)
    for n, n_parts, key_col in ((0, 3, 0), (1, 1, 0), (1000, 5, 2),
                                (4097, 64, 1)):
        cols = [rng.integers(-50, 50, size=n).astype(np.int64)
                for _ in range(3)]
        cols[0] = np.arange(n, dtype=np.int64)          # input row number
        if key_col == 0:
            cols[1] = cols[0].copy()
        cols.append(rng.random(n))                       # an f64 plane
        p = partition_host(cols, key_col, KEY_I64, n_parts)
        assert p.row_start[0] == 0 and p.row_start[-1] == n
        rows = p.cols[0] if key_col else p.cols[1]
        assert sorted(rows.tolist()) == list(range(n))   # a permutation
        for c, oc in zip(cols, p.cols):
            assert oc.dtype == c.dtype
            assert np.array_equal(oc, c[rows])           # rows move whole
        key = cols[key_col]
        for q in range(n_parts):
            seg = p.part_cols(q)
            r = (seg[0] if key_col else seg[1]).tolist()
            assert r == sorted(r) and len(set(r)) == len(r)   # stable
            assert all(owner_py(splitmix64_py(int(k) & M64), n_parts) == q
                       for k in key[r])


def test_utf8_segments_are_standalone_arrays():
    rng = np.random.default_rng(7)
    strs = [rng.integers(0, 256, size=int(ln), dtype=np.uint8).tobytes()
            for ln in rng.integers(0, 20, size=300)]
    strs[17] = b""
    strs[18] = b"a\x00b"
    off, data = strings_to_arrow(strs)
    # a slice of a larger array: offsets[0] != 0
    off2 = (off + 11).astype(np.int32)
    data2 = np.concatenate([np.full(11, 0xEE, np.uint8), data,
                            np.full(5, 0xEE, np.uint8)])
    hashes = rng.integers(0, 1 << 63, size=300, dtype=np.uint64) * 2 + 1
    for n_parts in (1, 3, 8):
        p = partition_host([hashes, np.arange(300)], 0, KEY_HASH, n_parts,
                           utf8=(off2, data2))
        assert len(p.utf8_offsets) == 300 + n_parts
        assert p.byte_start[0] == 0 and p.byte_start[-1] == len(data)
        assert len(p.utf8_data) == len(data)
        for q in range(n_parts):
            o, d = p.part_utf8(q)
            assert o[0] == 0 and len(o) == p.count(q) + 1
            assert o[-1] == len(d) == p.byte_start[q + 1] - p.byte_start[q]
            rows = p.part_cols(q)[1].tolist()
            assert arrow_to_strings(o, d) == [strs[r] for r in rows]


N_ROWS = 3000


def _source_batch(rank, world):
    """The batch rank `rank` contributes: strings, their stand-in content
    hash (any pure function of the bytes will do on the host) and a row id."""
    rng = np.random.default_rng(100 + rank)
    pool = [b"key-%d-%s" % (i, b"x" * (i % 9)) for i in range(40)] + [b""]
    strs = [pool[i] for i in rng.integers(0, len(pool), size=N_ROWS)]
    hashes = np.array(
        [splitmix64_py(int.from_bytes(s[:8].ljust(8, b"\x01"), "little") ^
                       len(s)) for s in strs], dtype=np.uint64)
    rowid = np.arange(N_ROWS, dtype=np.int64) + rank * 1_000_000
    return strs, hashes, rowid


def _rank_main(rank, world, port, q, on_device=False):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    strs, hashes, rowid = _source_batch(rank, world)
    off, data = strings_to_arrow(strs)
    if on_device:
        # every rank partitions on device 0 with its own handle; the
        # exchange itself stays on gloo
        import torch
        torch.cuda.init()
        from arroyo_amd import cabi, gpu
        dev = torch.device("cuda", 0)
        sh = gpu.make_shuffler(cabi.make_shuffle_config(
            world, 2, key_col=0, key_mode=KEY_HASH, has_utf8=True,
            max_rows=N_ROWS, max_bytes=len(data)))
        to_dev = lambda a: torch.from_numpy(a).to(dev)
        recv = shuffle_batch([to_dev(hashes), to_dev(rowid)], 0, KEY_HASH,
                             world, utf8=(to_dev(off), to_dev(data)),
                             partitioner=sh)
        sh.close()
    else:
        recv = shuffle_batch([hashes, rowid], 0, KEY_HASH, world,
                             utf8=(off, data))
    out = []
    for cols, (off, data) in recv:
        out.append((cols[0].numpy().view(np.uint64).tolist(),
                    cols[1].numpy().tolist(),
                    arrow_to_strings(off.numpy(), data.numpy())))
    q.put((rank, out))
    dist.destroy_process_group()


def _run_two_ranks(port, on_device):
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_rank_main,
                         args=(r, world, port, q, on_device))
             for r in range(world)]
    for p in procs:
        p.start()
    results = dict(q.get(timeout=300) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0

    sent = Counter()
    got = Counter()
    for src in range(world):
        strs, hashes, rowid = _source_batch(src, world)
        sent.update(zip(strs, rowid.tolist()))
        for dst in range(world):
            h, rows, rs = results[dst][src]
            # exactly the rows dst owns, in the source's order
            mine = [i for i in range(N_ROWS)
                    if owner_py(int(hashes[i]), world) == dst]
            assert rows == [int(rowid[i]) for i in mine]
            assert rs == [strs[i] for i in mine]
            assert h == [int(hashes[i]) for i in mine]
            got.update(zip(rs, rows))
    assert got == sent
    owners = [{s for src in range(world) for s in results[dst][src][2]}
              for dst in range(world)]
    assert not (owners[0] & owners[1])
    assert all(len(o) > 5 for o in owners)


def test_two_rank_shuffle_batch_with_utf8_column():
    _run_two_ranks(29461, on_device=False)


@pytest.mark.gpu
def test_two_rank_shuffle_batch_device_partitioner():
    """The same exchange with gpu.Shuffler as the partitioner on each rank."""
    _run_two_ranks(29467, on_device=True)
