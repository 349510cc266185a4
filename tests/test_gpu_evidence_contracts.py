"""What ampli_pileup_evidence and ampli_evidence_score write, on poisoned and fenced buffers (helpers.fenced): the count ADDS to the bins
it owns and touches nothing else -- not a bin whose sum is zero, not a byte in front of or behind either output --, the calls the contract
names no-ops write nothing at all, and the score overwrites every output cell and writes none of its inputs."""
import ctypes as C

import numpy as np
import pytest

from tests import evidence_model as em
from tests import helpers

pytestmark = pytest.mark.gpu
BY_NAME = {c.name: c for c in em.cases()}
POISON = -1  # 0xFF bytes as int32 / int64


def _fenced(P):
    import torch

    return helpers.fenced((P, 4, em.METRICS, em.BINS), torch.int32), helpers.fenced((2,), torch.int64)


@pytest.mark.parametrize("name", ["walk_across_2000_positions_dense", "walk_across_2000_positions_sparse", "the_windows_last_key_and_the_first_beyond", "list_of_1_keys",
                                  "keys_at_the_top_of_the_coordinate_range", f"fuzz_{em.FUZZ_SEEDS[1]}_1777_reads_sparse", f"fuzz_{em.FUZZ_SEEDS[1]}_1777_reads_dense"])
def test_a_call_adds_to_its_bins_and_to_nothing_else(ctx, name):
    case = BY_NAME[name]
    (hist, check_hist), (stats, check_stats) = _fenced(len(case.keys))
    ctx.read_evidence(*em.upload(case), mbq=case.mbq, mrq=case.mrq, hist=hist, stats=stats)
    got = em.device_result(ctx, hist, stats)
    w = case.want()
    assert np.array_equal(got.hist, POISON + w.hist)  # added to what was there; every zero sum keeps the poison
    assert got.stats == (POISON + w.stats[0], POISON + w.stats[1])
    check_hist(), check_stats()


def test_the_no_op_calls_write_nothing(ctx):
    case = BY_NAME["walk_across_2000_positions_sparse"]
    P = len(case.keys)
    (hist, check_hist), (stats, check_stats) = _fenced(P)
    bam, off, keys = em.upload(case)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    call = ctx.lib.ampli_pileup_evidence
    assert call(ctx.h, p(bam), p(off), 0, p(keys), P, 20, 20, p(hist), p(stats)) == 0             # no reads
    assert call(ctx.h, p(bam), p(off), case.n_reads, p(keys), 0, 20, 20, p(hist), p(stats)) == 0  # no positions
    empty = em.Case("nothing_kept", [dict(r, mapq=0) for r in case.reads[:300]], case.keys)        # reads, but none kept
    assert empty.want().stats == (0, 0)
    ctx.read_evidence(*em.upload(empty), mbq=20, mrq=20, hist=hist, stats=stats)
    got = em.device_result(ctx, hist, stats)
    assert np.all(got.hist == POISON) and got.stats == (POISON, POISON)
    check_hist(), check_stats()


def test_the_score_overwrites_every_output_cell_and_writes_no_input(ctx):
    import torch

    planes, ref, alt = em.random_planes(np.random.default_rng(2906), 333)
    P = len(planes)
    # the inputs in fenced buffers of their own, filled behind the poison: a store into them or next to them shows
    (hist, check_hist), (d_ref, check_ref), (d_alt, check_alt) = helpers.fenced(planes.shape, torch.int32), helpers.fenced((P,), torch.int8), helpers.fenced((P,), torch.int8)
    hist.copy_(torch.from_numpy(planes.astype(np.int32)))
    d_ref.copy_(torch.from_numpy(ref.astype(np.int8)))
    d_alt.copy_(torch.from_numpy(alt.astype(np.int8)))
    want = em.score(planes, ref, alt)
    assert (want.ints[:, :, 2] < 0).any() and (want.alt_used < 0).any() and (want.med < 0).any()  # untested cells are among them
    for poison in (0xFF, 0x55):  # -1 is a value of an untested cell: the second poison is none of anything
        (ints, check_ints), (med, check_med) = helpers.fenced((P, em.METRICS, 3), torch.int64, poison), helpers.fenced((P, em.METRICS, 2), torch.int32, poison)
        (z2, check_z2), (used, check_used) = helpers.fenced((P, em.METRICS), torch.float64, poison), helpers.fenced((P,), torch.int8, poison)
        ctx.evidence_score(hist, d_ref, d_alt, ints=ints, med=med, z2=z2, alt_used=used)
        ctx.sync()
        torch.cuda.synchronize()
        found = em.score_differences(em.Score(ints.cpu().numpy(), med.cpu().numpy(), z2.cpu().numpy(), used.cpu().numpy()), want)
        assert not found, found  # every cell holds its value: none kept the poison
        assert np.array_equal(hist.cpu().numpy(), planes) and np.array_equal(d_ref.cpu().numpy(), ref) and np.array_equal(d_alt.cpu().numpy(), alt)
        for check in (check_hist, check_ref, check_alt, check_ints, check_med, check_z2, check_used):
            check()
