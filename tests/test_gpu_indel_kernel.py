"""ampli_pileup_indel_count itself (through Context.indel_count), one call per case of the table of tests/indel_model.py, against the
model: exact integer equality of the counts, the length bins and the stats; the same without the length plane; halves of a stream
that accumulate to the whole; the argument checks."""
import ctypes as C
import time

import numpy as np
import pytest

from tests import indel_model as im

pytestmark = pytest.mark.gpu
CASES = im.cases()
BY_NAME = {c.name: c for c in CASES}


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_counts_lengths_and_stats_equal_the_model(ctx, case):
    t0 = time.perf_counter()
    got = im.device_result(ctx, *ctx.indel_count(*im.upload(case), mbq=case.mbq, mrq=case.mrq))
    want = case.want()
    print(f"{case!r}: {time.perf_counter() - t0:.3f} s incl. upload and model; stats {got.stats}, insertions {int(got.counts[:, 1].sum())}, deletions {int(got.counts[:, 2].sum())}")
    found = im.differences(got, want)
    assert not found, found


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_the_same_without_the_length_plane(ctx, case):
    counts, lengths, stats = ctx.indel_count(*im.upload(case), mbq=case.mbq, mrq=case.mrq, lengths=False)
    assert lengths is None
    found = im.differences(im.device_result(ctx, counts, None, stats), case.want(), lengths=False)
    assert not found, found


@pytest.mark.parametrize("name", ["walk_across_2000_positions", "reads_in_random_order", "257_reads_with_one_junction", f"fuzz_{im.FUZZ_SEEDS[0]}_3000_reads"])
def test_two_calls_on_halves_accumulate_to_the_whole(ctx, name):
    case = BY_NAME[name]
    half = case.n_reads // 2 + 1
    out = ctx.indel_count(*im.upload(case, 0, half), mbq=case.mbq, mrq=case.mrq)
    out = ctx.indel_count(*im.upload(case, half, None), mbq=case.mbq, mrq=case.mrq, counts=out[0], lengths=out[1], stats=out[2])
    found = im.differences(im.device_result(ctx, *out), case.want())
    assert case.want().stats[1] > 0 and not found, found


def test_the_same_call_twice_doubles_everything(ctx):
    case = BY_NAME["walk_across_2000_positions"]
    args = im.upload(case)
    out = ctx.indel_count(*args, mbq=case.mbq, mrq=case.mrq)
    out = ctx.indel_count(*args, mbq=case.mbq, mrq=case.mrq, counts=out[0], lengths=out[1], stats=out[2])
    w = case.want()
    found = im.differences(im.device_result(ctx, *out), im.Result(2 * w.counts, 2 * w.lengths, (2 * w.stats[0], 2 * w.stats[1])))
    assert not found, found


def test_without_a_stats_buffer(ctx):
    case = BY_NAME["holes_in_the_panel"]
    counts, lengths, stats = ctx.indel_count(*im.upload(case), mbq=case.mbq, mrq=case.mrq, stats=False)
    assert stats is None
    found = im.differences(im.device_result(ctx, counts, lengths, None), case.want(), stats=False)
    assert not found, found


def test_argument_checks(ctx):
    import torch

    case = BY_NAME["insertion_forward_10M2I10M"]
    bam, off, keys = im.upload(case)
    P, n = keys.numel(), off.numel()
    counts = torch.zeros((P, 8), dtype=torch.int32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    call = ctx.lib.ampli_pileup_indel_count
    INVALID = ctx.lib.ampli_pileup_count(ctx.h, None, None, 0, None, 0, 20, 20, None, None)  # the existing "bad argument" code
    assert INVALID != 0
    good = (ctx.h, p(bam), p(off), n, p(keys), P, 20, 20, p(counts), None, None)
    for at, bad in ((1, None), (2, None), (3, -1), (4, None), (5, -1), (8, None)):
        args = list(good)
        args[at] = bad
        assert call(*args) == INVALID, at
        assert b"pileup_indel_count: bad argument" in ctx.lib.ampli_last_error(ctx.h)
    assert call(None, *good[1:]) == INVALID
    ctx.sync()
    assert int(counts.abs().sum()) == 0  # no refused call counted anything
    assert call(*good) == 0
    ctx.sync()
    assert np.array_equal(counts.cpu().numpy().astype(np.int64), case.want().counts)


def test_misaligned_pointers_are_refused_before_anything_is_launched(ctx):
    """d_rec_off, d_keys and d_stats below 8 bytes, d_counts and d_lengths below 4: AMPLI_E_INVALID, and the fenced outputs are untouched"""
    import torch

    from tests.helpers import assert_misaligned_refused, fenced

    case = BY_NAME["insertion_forward_10M2I10M"]
    bam, off, keys = im.upload(case)
    P = keys.numel()
    counts, lengths, stats = fenced((P, 8), torch.int32), fenced((P, 2, im.BINS), torch.int32), fenced((2,), torch.int64)
    good = (ctx.h, bam.data_ptr(), off.data_ptr(), off.numel(), keys.data_ptr(), P, 20, 20, counts[0].data_ptr(), lengths[0].data_ptr(), stats[0].data_ptr())
    assert_misaligned_refused(ctx, ctx.lib.ampli_pileup_indel_count, good, [(2, 4), (4, 4), (8, 2), (9, 2), (10, 4)], [counts, lengths, stats],
                              b"pileup_indel_count: bad argument")
