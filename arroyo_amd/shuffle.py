"""Keyed shuffle exchange between ranks (the MI355X-native equivalent of the
reference's cross-subtask repartition: crates/arroyo-operator/src/context.rs:
506-560 `repartition` + crates/arroyo-worker/src/network_manager.rs Arrow-IPC
transport).

Partitioning matches the reference's scheme: 64-bit hash of the key column,
owner = contiguous u64 range (server_for_hash,
crates/arroyo-types/src/lib.rs:640-647).  The hash itself is splitmix64, not
ahash — allowed because both ends of our shuffle use it consistently and
result parity does not depend on partition assignment.

Exchange primitive:
  - RCCL (backend "nccl" on ROCm): one fused `all_to_all_single` per column
    over xGMI — every GPU pair has a direct link, so all-to-all is the natural
    collective.
  - gloo (CPU tests): gloo supports neither all_to_all nor all_to_all_single,
    so the same exchange runs as point-to-point isend/irecv pairs.
"""
import numpy as np
import torch
import torch.distributed as dist

SPLITMIX_C1 = 0x9E3779B97F4A7C15
SPLITMIX_C2 = 0xBF58476D1CE4E5B9
SPLITMIX_C3 = 0x94D049BB133111EB
U64 = np.uint64


def splitmix64_np(x):
    x = x.astype(U64) + U64(SPLITMIX_C1)
    x = (x ^ (x >> U64(30))) * U64(SPLITMIX_C2)
    x = (x ^ (x >> U64(27))) * U64(SPLITMIX_C3)
    return x ^ (x >> U64(31))


def tuple_hash_np(cols, valid=None):
    """The content hash of the tuple-key dictionary (arroyo_amd_tuplekey_*),
    restated in numpy: h = splitmix64(mask), then h = splitmix64(h ^ w_c)
    for every component in order, with bit c of mask set and w_c = 0 where
    component c is NULL.  cols: equal-length 8-byte numpy columns, taken as
    raw bits; valid: None or a list parallel to cols of None (all valid) /
    bool masks (True = non-null).  The sending side of a keyed shuffle can
    hash on the host with it and partition in KEY_HASH mode."""
    words = []
    for c in cols:
        c = np.ascontiguousarray(c)
        if c.dtype.itemsize != 8:
            raise ValueError("tuple components are 8-byte elements")
        words.append(c.view(U64))
    n = len(words[0]) if words else 0
    mask = np.zeros(n, dtype=U64)
    for i, w in enumerate(words):
        if valid is None or valid[i] is None:
            continue
        null = ~np.asarray(valid[i], dtype=bool)
        mask |= null.astype(U64) << U64(i)
        words[i] = np.where(null, U64(0), w)
    with np.errstate(over="ignore"):
        h = splitmix64_np(mask)
        for w in words:
            h = splitmix64_np(h ^ w)
    return h


def partition_ids(keys, n_parts):
    """Owner rank per row: hash / (2^64 / n) — contiguous hash ranges, same
    scheme as server_for_hash (arroyo-types:640-647)."""
    with np.errstate(over="ignore"):
        h = splitmix64_np(np.asarray(keys).astype(np.int64).view(np.uint64)
                          if np.asarray(keys).dtype != np.uint64
                          else np.asarray(keys))
    range_size = U64(2**64 // n_parts)
    return (h // range_size).astype(np.int64)


KEY_I64 = 0    # cabi.AMD_SHUF_KEY_I64: owner from splitmix64 of the key column
KEY_HASH = 1   # cabi.AMD_SHUF_KEY_HASH: the key column already is a hash


def owners_device_rule(h, n_parts):
    """Owner per 64-bit hash by the device rule (k_partition and the
    arroyo_amd_shuffle_* family): range = UINT64_MAX // n_parts + 1,
    owner = h // range, owner = 0 for one partition.  Unlike partition_ids'
    2**64 // n_parts this never yields owner == n_parts."""
    h = np.asarray(h, dtype=np.uint64)
    if n_parts == 1:
        return np.zeros(len(h), dtype=np.int64)
    return (h // U64((2**64 - 1) // n_parts + 1)).astype(np.int64)


class Partitioned:
    """A batch split into n_parts contiguous segments, rows of a segment in
    input order: the layout of AmdShuffleOut.  cols, utf8_offsets and
    utf8_data are numpy arrays (partition_host) or torch device tensors
    (gpu.Shuffler.partition); row_start and byte_start are host int lists
    of n_parts + 1 entries."""

    def __init__(self, cols, row_start, utf8_offsets=None, utf8_data=None,
                 byte_start=None):
        self.cols = cols
        self.row_start = [int(x) for x in row_start]
        self.utf8_offsets = utf8_offsets
        self.utf8_data = utf8_data
        self.byte_start = [int(x) for x in byte_start] \
            if byte_start is not None else [0] * len(self.row_start)
        self.n_parts = len(self.row_start) - 1

    def count(self, p):
        return self.row_start[p + 1] - self.row_start[p]

    def part_cols(self, p):
        lo, hi = self.row_start[p], self.row_start[p + 1]
        return [c[lo:hi] for c in self.cols]

    def part_utf8(self, p):
        """Partition p's strings as a standalone Arrow Utf8 array:
        (count + 1 offsets starting at 0, its bytes)."""
        if self.utf8_offsets is None:
            return None
        lo, hi = self.row_start[p] + p, self.row_start[p + 1] + p + 1
        return (self.utf8_offsets[lo:hi],
                self.utf8_data[self.byte_start[p]:self.byte_start[p + 1]])


def partition_host(cols, key_col, key_mode, n_parts, utf8=None):
    """numpy restatement of arroyo_amd_shuffle_partition_device: device owner
    rule, then a stable argsort.  cols: equal-length 8-byte numpy columns;
    utf8: (int32 offsets [n + 1], uint8 data) or None.  The checker for the
    kernels and the CPU path of shuffle_batch."""
    cols = [np.ascontiguousarray(c) for c in cols]
    for c in cols:
        if c.dtype.itemsize != 8:
            raise ValueError("shuffle columns are 8-byte elements")
    key = cols[key_col].view(np.uint64)
    with np.errstate(over="ignore"):
        h = key if key_mode == KEY_HASH else splitmix64_np(key)
    owner = owners_device_rule(h, n_parts)
    order = np.argsort(owner, kind="stable")
    row_start = np.zeros(n_parts + 1, dtype=np.int64)
    np.cumsum(np.bincount(owner, minlength=n_parts), out=row_start[1:])
    out_cols = [c[order] for c in cols]
    if utf8 is None:
        return Partitioned(out_cols, row_start)
    offsets = np.asarray(utf8[0]).astype(np.int64)
    data = np.asarray(utf8[1], dtype=np.uint8)
    if len(offsets) != len(order) + 1:
        raise ValueError("offsets needs n_rows + 1 entries")
    lens = np.diff(offsets)
    if offsets[0] < 0 or (lens < 0).any():
        raise ValueError("malformed offsets: negative or decreasing")
    lens = lens[order]
    pos = np.zeros(len(order) + 1, dtype=np.int64)   # destination byte of row
    np.cumsum(lens, out=pos[1:])
    byte_start = pos[row_start]
    out_off = np.empty(len(order) + n_parts, dtype=np.int32)
    for p in range(n_parts):
        lo, hi = row_start[p], row_start[p + 1]
        out_off[lo + p:hi + p + 1] = pos[lo:hi + 1] - byte_start[p]
    src = np.repeat(offsets[:-1][order] - pos[:-1], lens) + \
        np.arange(pos[-1], dtype=np.int64)
    return Partitioned(out_cols, row_start, out_off, data[src], byte_start)


def shuffle_batch(cols, key_col, key_mode, n_parts, utf8=None, group=None,
                  partitioner=None):
    """Stable keyed exchange of one batch: partition (partitioner.partition,
    a gpu.Shuffler, on torch device tensors; partition_host on numpy columns
    otherwise), then all_to_all_tensors per column and, with utf8, for the
    offsets and the bytes.  Returns what was received PER SOURCE RANK, in
    rank order, as a list of (cols, utf8) with utf8 = (offsets, data) or
    None: every source's rows stay in its order, so the result does not
    depend on arrival order."""
    world = dist.get_world_size(group)
    assert world == n_parts
    if partitioner is not None:
        part = partitioner.partition(cols, utf8)
        # RCCL sends the device segments as they are; any other backend
        # (gloo) gets host copies
        if dist.get_backend(group) == "nccl":
            as_tensor = lambda x: x
        else:
            as_tensor = lambda x: x.cpu()
    else:
        part = partition_host(cols, key_col, key_mode, n_parts, utf8)
        as_tensor = lambda x: torch.from_numpy(np.ascontiguousarray(x))
    recv_cols = []
    for c in range(len(part.cols)):
        recv_cols.append(all_to_all_tensors(
            [as_tensor(part.part_cols(p)[c]) for p in range(n_parts)], group))
    recv_off = recv_data = None
    if part.utf8_offsets is not None:
        segs = [part.part_utf8(p) for p in range(n_parts)]
        recv_off = all_to_all_tensors([as_tensor(s[0]) for s in segs], group)
        recv_data = all_to_all_tensors([as_tensor(s[1]) for s in segs], group)
    return [([rc[src] for rc in recv_cols],
             (recv_off[src], recv_data[src]) if recv_off is not None else None)
            for src in range(world)]


def recv_splits_of(gathered_flat, world, rank):
    """Decode an all-gathered [world x world] send-split matrix (row =
    sender, column = destination) into this rank's receive splits, indexed
    by source rank.  Shared by bench.py's RCCL exchange and the
    single-process bookkeeping test."""
    return [int(gathered_flat[src * world + rank]) for src in range(world)]


def exchange_sizes(send_counts, group=None):
    """All-gather the per-destination row counts; returns recv_counts[src]."""
    world = dist.get_world_size(group)
    rank = dist.get_rank(group)
    t = torch.tensor(send_counts, dtype=torch.int64)
    gathered = [torch.zeros_like(t) for _ in range(world)]
    dist.all_gather(gathered, t, group=group)
    return [int(gathered[src][rank]) for src in range(world)]


def all_to_all_tensors(send, group=None):
    """Exchange a list of per-destination 1-D tensors; returns the received
    list indexed by source rank.  Works on gloo (isend/irecv) and nccl/RCCL
    (all_to_all_single over xGMI)."""
    world = dist.get_world_size(group)
    rank = dist.get_rank(group)
    assert len(send) == world
    recv_counts = exchange_sizes([s.numel() for s in send], group)
    backend = dist.get_backend(group)
    if backend == "nccl":
        send_flat = torch.cat([s for s in send])
        recv_flat = send_flat.new_empty(sum(recv_counts))
        dist.all_to_all_single(
            recv_flat, send_flat,
            output_split_sizes=recv_counts,
            input_split_sizes=[s.numel() for s in send], group=group)
        out, off = [], 0
        for c in recv_counts:
            out.append(recv_flat[off:off + c])
            off += c
        return out
    # gloo: point-to-point. Self-row is a local copy; peers paired isend/irecv.
    out = [None] * world
    out[rank] = send[rank].clone()
    reqs = []
    recvs = {}
    for peer in range(world):
        if peer == rank:
            continue
        if send[peer].numel():
            reqs.append(dist.isend(send[peer].contiguous(), dst=peer,
                                   group=group, tag=0))
        if recv_counts[peer]:
            buf = send[rank].new_empty(recv_counts[peer])
            recvs[peer] = buf
            reqs.append(dist.irecv(buf, src=peer, group=group, tag=0))
    for r in reqs:
        r.wait()
    for peer in range(world):
        if peer == rank:
            continue
        out[peer] = recvs.get(peer, send[rank].new_empty(0))
    return out


def shuffle_columns(cols, n_parts, group=None):
    """Repartition a batch (list of equal-length int64 numpy columns, key col
    first) across ranks by key-hash range; returns the merged received
    columns.  CPU/gloo path; the GPU path does the partition+scatter on
    device (arroyo_amd_partition) and exchanges device buffers over RCCL."""
    world = dist.get_world_size(group)
    assert world == n_parts
    pid = partition_ids(cols[0], n_parts)
    order = np.argsort(pid, kind="stable")
    counts = np.bincount(pid, minlength=n_parts)
    merged = []
    for c in cols:
        sorted_c = np.ascontiguousarray(np.asarray(c)[order])
        send, off = [], 0
        for p in range(n_parts):
            send.append(torch.from_numpy(
                sorted_c[off:off + counts[p]].copy()))
            off += counts[p]
        recv = all_to_all_tensors(send, group)
        merged.append(torch.cat(recv).numpy())
    return merged
