"""What ampli_pileup_phase (C33) and ampli_phase_score (C34) write, on poisoned and fenced buffers (helpers.fenced): the count ADDS to the
cells it owns and touches nothing else -- not a cell whose sum is zero, not a cell with i + 1 + k >= P, not a byte in front of or behind
either output --, the calls the contract names no-ops write nothing at all, and the score overwrites every output cell and writes none of
its inputs."""
import ctypes as C

import numpy as np
import pytest

from tests import helpers
from tests import phase_model as ph

pytestmark = pytest.mark.gpu
BY_NAME = {c.name: c for c in ph.cases()}
POISON = -1  # 0xFF bytes as int32 / int64
SHAPE = (ph.K, ph.STATES, ph.STATES)


def _fenced(P):
    import torch

    return helpers.fenced((P,) + SHAPE, torch.int32), helpers.fenced((3,), torch.int64)


@pytest.mark.parametrize("name", ["a_stream_in_descending_position_order_dense", "a_stream_in_ascending_position_order_sparse",
                                  "the_windows_last_key_with_the_first_beyond_and_pairs_wholly_beyond", "nine_keys_inside_one_read", "keys_on_two_references",
                                  f"fuzz_{ph.FUZZ_SEEDS[1]}_777_reads_sparse", f"fuzz_{ph.FUZZ_SEEDS[1]}_777_reads_dense"])
def test_a_call_adds_to_its_cells_and_to_nothing_else(ctx, name):
    from amplisolve_amd import read_phase

    case = BY_NAME[name]
    P = len(case.keys)
    (table, check_table), (stats, check_stats) = _fenced(P)
    read_phase(ctx, *ph.upload(case), mbq=case.mbq, mrq=case.mrq, table=table, stats=stats)
    got = ph.device_result(ctx, table, stats)
    w = case.want()
    assert np.array_equal(got.table, POISON + w.table)  # added to what was there; every zero sum keeps the poison
    assert got.stats == tuple(POISON + x for x in w.stats)
    beyond = np.add.outer(np.arange(P), np.arange(ph.K)) + 1 >= P  # the cells with i + 1 + k >= P
    assert beyond.sum() == ph.K * (ph.K + 1) // 2 or P <= ph.K
    assert np.all(got.table[beyond] == POISON)
    check_table(), check_stats()


def test_the_no_op_calls_write_nothing(ctx):
    from amplisolve_amd import read_phase

    case = BY_NAME["a_stream_in_ascending_position_order_sparse"]
    P = len(case.keys)
    (table, check_table), (stats, check_stats) = _fenced(P)
    bam, off, keys = ph.upload(case)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    call = ctx.lib.ampli_pileup_phase
    assert call(p(bam), p(off), 0, p(keys), P, 20, 20, p(table), p(stats), ctx.h) == 0             # no reads
    assert call(p(bam), p(off), case.n_reads, p(keys), 0, 20, 20, p(table), p(stats), ctx.h) == 0  # no positions
    empty = ph.Case("nothing_kept", [dict(r, mapq=0) for r in case.reads[:300]], case.keys)        # reads, but none kept
    assert empty.want().stats == (0, 0, 0)
    read_phase(ctx, *ph.upload(empty), mbq=20, mrq=20, table=table, stats=stats)
    one_key = ph.Case("every_read_covers_one_key", case.reads[:300], case.keys[:1])                # reads kept, no pair
    assert one_key.want().stats[0] == 300 and one_key.want().stats[1:] == (0, 0)
    (t1, check_t1), (s1, check_s1) = _fenced(1)
    read_phase(ctx, *ph.upload(one_key), mbq=20, mrq=20, table=t1, stats=s1)
    got, got1 = ph.device_result(ctx, table, stats), ph.device_result(ctx, t1, s1)
    assert np.all(got.table == POISON) and got.stats == (POISON,) * 3
    assert np.all(got1.table == POISON) and got1.stats == (POISON + 300, POISON, POISON)
    check_table(), check_stats(), check_t1(), check_s1()


def test_the_score_overwrites_every_output_cell_and_writes_no_input(ctx):
    import torch

    from amplisolve_amd import phase_score

    t, cells, nts = ph.random_tables(np.random.default_rng(3206), 40)
    Q = len(cells)
    # the inputs in fenced buffers of their own, filled behind the poison: a store into them or next to them shows
    (table, check_table), (d_cell, check_cell), (d_nt, check_nt) = helpers.fenced(t.shape, torch.int32), helpers.fenced((Q,), torch.int64), helpers.fenced((Q, 4), torch.int8)
    table.copy_(torch.from_numpy(t.astype(np.int32)))
    d_cell.copy_(torch.from_numpy(cells.astype(np.int64)))
    d_nt.copy_(torch.from_numpy(nts.astype(np.int8)))
    want = ph.score(t, cells, nts)
    assert (want.cls < 0).sum() >= 20 and (want.cls > 0).any() and (cells < 0).any() and (cells >= len(t) * ph.K).any()  # untested pairs are among them
    for poison in (0xFF, 0x55):  # -1 is a value of an untested pair: the second poison is none of anything
        (ints, check_ints), (score, check_score), (cls, check_cls) = helpers.fenced((Q, 6), torch.int64, poison), helpers.fenced((Q,), torch.float32, poison), helpers.fenced((Q,), torch.int32, poison)
        phase_score(ctx, table, d_cell, d_nt, ints=ints, score=score, cls=cls)
        ctx.sync()
        torch.cuda.synchronize()
        found = ph.score_differences(ph.Score(ints.cpu().numpy(), score.cpu().numpy(), cls.cpu().numpy(), None), want)
        assert not found, found  # every cell holds its value: none kept the poison
        assert np.array_equal(table.cpu().numpy(), t) and np.array_equal(d_cell.cpu().numpy(), cells) and np.array_equal(d_nt.cpu().numpy(), nts)
        for check in (check_table, check_cell, check_nt, check_ints, check_score, check_cls):
            check()
