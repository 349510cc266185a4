"""What ampli_pileup_indel_count writes, on poisoned and fenced buffers (helpers.fenced): it ADDS to the counters it owns and touches
nothing else -- not slots 3 and 7, not a counter whose sum is zero, not a byte in front of or behind any of its three outputs -- and
the calls the contract names no-ops write nothing at all."""
import ctypes as C

import numpy as np
import pytest

from tests import helpers
from tests import indel_model as im

pytestmark = pytest.mark.gpu
BY_NAME = {c.name: c for c in im.cases()}
POISON = -1  # 0xFF bytes as int32 / int64


def _fenced(P):
    import torch

    return helpers.fenced((P, 8), torch.int32), helpers.fenced((P, 2, im.BINS), torch.int32), helpers.fenced((2,), torch.int64)


@pytest.mark.parametrize("name", ["walk_across_2000_positions", "event_just_outside_the_window", "panel_of_1_positions", "length_1000",
                                  "keys_at_the_top_of_the_coordinate_range", f"fuzz_{im.FUZZ_SEEDS[1]}_1777_reads"])
@pytest.mark.parametrize("with_lengths", [True, False])
def test_a_call_adds_to_its_counters_and_to_nothing_else(ctx, name, with_lengths):
    case = BY_NAME[name]
    (counts, check_counts), (lengths, check_lengths), (stats, check_stats) = _fenced(len(case.keys))
    ctx.indel_count(*im.upload(case), mbq=case.mbq, mrq=case.mrq, counts=counts, lengths=lengths if with_lengths else False, stats=stats)
    got = im.device_result(ctx, counts, lengths, stats)
    w = case.want()
    assert np.array_equal(got.counts, POISON + w.counts)  # added to what was there; slots 3 and 7 and every zero sum keep the poison
    assert np.all(got.counts[:, 3] == POISON) and np.all(got.counts[:, 7] == POISON)
    assert np.array_equal(got.lengths, POISON + (w.lengths if with_lengths else np.zeros_like(w.lengths)))  # untouched without the plane
    assert got.stats == (POISON + w.stats[0], POISON + w.stats[1])
    check_counts(), check_lengths(), check_stats()


def test_the_no_op_calls_write_nothing(ctx):
    case = BY_NAME["walk_across_2000_positions"]
    P = len(case.keys)
    (counts, check_counts), (lengths, check_lengths), (stats, check_stats) = _fenced(P)
    bam, off, keys = im.upload(case)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    call = ctx.lib.ampli_pileup_indel_count
    assert call(ctx.h, p(bam), p(off), 0, p(keys), P, 20, 20, p(counts), p(lengths), p(stats)) == 0                # no reads
    assert call(ctx.h, p(bam), p(off), case.n_reads, p(keys), 0, 20, 20, p(counts), p(lengths), p(stats)) == 0     # no positions
    empty = im.Case("nothing_kept", [dict(r, mapq=0) for r in case.reads[:300]], case.keys)                         # reads, but none kept
    assert empty.want().stats == (0, 0)
    ctx.indel_count(*im.upload(empty), mbq=20, mrq=20, counts=counts, lengths=lengths, stats=stats)
    got = im.device_result(ctx, counts, lengths, stats)
    assert np.all(got.counts == POISON) and np.all(got.lengths == POISON) and got.stats == (POISON, POISON)
    check_counts(), check_lengths(), check_stats()
