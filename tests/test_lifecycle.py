"""Create / use / close cycles of every operator but the window operator
(tests/test_errors.py::test_create_destroy_leak_free has that one) must give
their device memory back.

What this catches is a forgotten LARGE buffer: each case's configuration is
its smallest useful one, and the smallest buffer the bound can see is named
beside it -- over CYCLES = 20 cycles it comes to 160 MiB, well above the
64 MiB bound of the window operator's test, while allocator noise stays far
below it.  Small buffers (cursors, error words, key tables at log2 capacity
10 to 12) are below what free-memory readings resolve; that they go through
the handle's owner is checked by searching the sources for raw hipMalloc /
hipFree (profiles/op_common_note.md), not here.  Pinned host staging does
not show in device free memory either; its device twin does."""
import numpy as np
import pytest

from arroyo_amd import cabi

NS = 10**9
T0 = 1_600_000_000 * NS
U64MAX = (1 << 64) - 1
N = 1000
CYCLES = 20          # every case; none needed a lower count to stay quick
BOUND = 64 * 1024 * 1024

KEYS = np.arange(N, dtype=np.int64)
VALS = (KEYS * 7) % 101
# four instants of 250 rows: instant tables stay at their smallest sizes
TS4 = T0 + (KEYS % 4) * NS
# one second of event time: a single session per key under a 2 s gap
TS_MS = T0 + KEYS * 10**6
ZERO = np.zeros(N, dtype=np.int64)


def cycle_join(gpu):
    # smallest tracked buffer: one 8 MiB device staging column (2^20 rows)
    op = gpu.make_join_op(cabi.make_join_config(
        n_keys=1, n_left_vals=1, n_right_vals=1, log2_rows_cap=10,
        instants=16, log2_out_cap=12))
    op.process_batch(op.LEFT, [KEYS, VALS, TS4])
    op.process_batch(op.RIGHT, [KEYS, VALS, TS4])
    out = op.handle_watermark(U64MAX)
    assert len(out[0]) == N
    op.close()


def cycle_session(gpu):
    # smallest tracked buffer: one 8 MiB device staging column
    op = gpu.make_session_op(cabi.make_session_config(
        2 * NS, [(cabi.COUNT, -1)], n_keys=1, log2_capacity=10,
        log2_batch_capacity=10, log2_out_cap=12))
    op.process_batch([KEYS % 100, TS_MS])
    out = op.handle_watermark(U64MAX)
    assert len(out[0]) == 100
    op.close()


def _cycle_expjoin(gpu, updating):
    # smallest tracked buffer: one 8 MiB device staging column; expire()
    # rebuilds each side's chains, the mid-life release path
    op = gpu.make_expjoin_op(cabi.make_expjoin_config(
        NS, n_left_vals=1, n_right_vals=1, log2_capacity=12,
        log2_rows_cap=12, log2_out_cap=12, updating=updating))
    retract = [ZERO] if updating else []
    op.process_batch(op.LEFT, [KEYS, VALS] + retract + [TS_MS])
    out = op.process_batch(op.RIGHT, [KEYS, VALS] + retract + [TS_MS])
    assert len(out[0]) == N
    op.handle_watermark(T0 + 10 * NS)
    op.expire()
    op.close()


def cycle_expjoin(gpu):
    _cycle_expjoin(gpu, False)


def cycle_expjoin_updating(gpu):
    # one more staging column (is_retract) than the plain join
    _cycle_expjoin(gpu, True)


def cycle_updagg(gpu):
    # smallest tracked buffer: one 8 MiB device staging column
    op = gpu.make_updagg_op(cabi.make_updagg_config(
        [(cabi.COUNT, -1), (cabi.SUM, 0)], n_keys=1, n_value_cols=1,
        log2_capacity=10, log2_nodes=12, log2_out_cap=12))
    op.process_batch([KEYS % 100, VALS, ZERO])
    assert len(op.flush()[0]) == 100
    op.close()


def cycle_updagg_nullable_median(gpu):
    # as above, plus the ordered-aggregate arena, the validity masks and the
    # bitmap staging (the last is 128 KiB a column: not visible here)
    op = gpu.make_updagg_op(cabi.make_updagg_config(
        [(cabi.MEDIAN, 0)], n_keys=1, n_value_cols=1, log2_capacity=10,
        log2_nodes=12, log2_out_cap=12, null_semantics=True))
    op.process_batch_nullable([KEYS % 100, VALS, ZERO],
                              [None, KEYS % 3 != 0, None])
    cols, _valid = op.flush_with_validity()
    assert len(cols[0]) == 100
    op.close()


def cycle_windowfn(gpu):
    # smallest tracked buffer: one 8 MiB device staging column
    op = gpu.make_windowfn_op(cabi.make_windowfn_config(
        n_cols=2, part_col=-1, order=[(0, False)], limit=1,
        log2_rows_cap=10, instants=16, log2_out_cap=12))
    op.process_batch([VALS, TS4])
    out = op.handle_watermark(U64MAX)
    assert len(out[0]) == 4
    op.close()


def cycle_mapop(gpu):
    # every buffer is 8 MiB (capacity is fixed at 2^20 rows)
    op = gpu.make_map_op(cabi.make_map_config(
        n_in_cols=2, prog=[(cabi.MOP_ADD, 0, 1, 2)], out_reg=[2]))
    out = op.process_batch([KEYS, VALS])
    assert np.array_equal(out[0], KEYS + VALS)
    op.close()


def cycle_strkey(gpu):
    # smallest tracked buffer: the 8 MiB string arena; decode and drain use
    # call-local scratch, encode grows the per-batch scratch
    d = gpu.make_strkey(cabi.make_strkey_config(
        log2_capacity=12, arena_bytes=8 << 20))
    off, data = cabi.strings_to_arrow([b"key-%d" % (i % 100) for i in range(N)])
    ids = d.encode(off, data)
    assert len(np.unique(ids)) == 100
    assert len(d.drain()[0]) == 100
    d.close()


def cycle_shuffle(gpu):
    # smallest tracked buffer: one 8 MiB output column (max_rows = 2^20)
    import torch
    sh = gpu.make_shuffler(cabi.make_shuffle_config(
        n_parts=4, n_cols=2, max_rows=1 << 20), bind_output=False)
    cols = [torch.from_numpy(c).cuda() for c in (KEYS, VALS)]
    torch.cuda.synchronize()
    out = sh.partition_ptrs([c.data_ptr() for c in cols], N)
    assert out.row_start[4] == N
    sh.close()


CASES = [cycle_join, cycle_session, cycle_expjoin, cycle_expjoin_updating,
         cycle_updagg, cycle_updagg_nullable_median, cycle_windowfn,
         cycle_mapop, cycle_strkey, cycle_shuffle]


@pytest.mark.gpu
@pytest.mark.parametrize("cycle", CASES,
                         ids=lambda f: f.__name__.replace("cycle_", ""))
def test_operator_lifecycle_leak_free(cycle):
    import torch

    from arroyo_amd import gpu

    cycle(gpu)  # warm allocator/pools
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    for _ in range(CYCLES):
        cycle(gpu)
    torch.cuda.synchronize()
    free1, _ = torch.cuda.mem_get_info()
    leaked = free0 - free1
    print(f"{cycle.__name__}: free-memory drop {leaked / 2**20:.1f} MiB "
          f"over {CYCLES} cycles")
    assert leaked < BOUND, \
        f"leaked ~{leaked / 1e6:.1f} MB over {CYCLES} cycles"
