"""ampli_pileup_evidence and ampli_evidence_score themselves (through Context.read_evidence / evidence_score), one call per case of the
table of tests/evidence_model.py, against the model: exact integer equality of every bin and of the stats; halves of a stream that
accumulate to the whole; the argument checks and no-ops; the score kernel on the model's planes, integers equal and z2 bit for bit."""
import ctypes as C
import time

import numpy as np
import pytest

from tests import evidence_model as em

pytestmark = pytest.mark.gpu
CASES = em.cases()
BY_NAME = {c.name: c for c in CASES}
SCORE_CASES = em.score_cases()


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_bins_and_stats_equal_the_model(ctx, case):
    t0 = time.perf_counter()
    got = em.device_result(ctx, *ctx.read_evidence(*em.upload(case), mbq=case.mbq, mrq=case.mrq))
    want = case.want()
    print(f"{case!r}: {time.perf_counter() - t0:.3f} s incl. upload and model; stats {got.stats}")
    found = em.differences(got, want)
    assert not found, found


@pytest.mark.parametrize("name", ["walk_across_2000_positions_dense", "walk_across_2000_positions_sparse", "reads_in_random_order", "257_reads",
                                  f"fuzz_{em.FUZZ_SEEDS[0]}_3000_reads_sparse", f"fuzz_{em.FUZZ_SEEDS[0]}_3000_reads_dense"])
def test_two_calls_on_halves_accumulate_to_the_whole(ctx, name):
    case = BY_NAME[name]
    half = case.n_reads // 2 + 1
    out = ctx.read_evidence(*em.upload(case, 0, half), mbq=case.mbq, mrq=case.mrq)
    out = ctx.read_evidence(*em.upload(case, half, None), mbq=case.mbq, mrq=case.mrq, hist=out[0], stats=out[1])
    found = em.differences(em.device_result(ctx, *out), case.want())
    assert case.want().stats[1] > 0 and not found, found


def test_the_same_call_twice_doubles_everything(ctx):
    case = BY_NAME["walk_across_2000_positions_sparse"]
    args = em.upload(case)
    out = ctx.read_evidence(*args, mbq=case.mbq, mrq=case.mrq)
    out = ctx.read_evidence(*args, mbq=case.mbq, mrq=case.mrq, hist=out[0], stats=out[1])
    w = case.want()
    found = em.differences(em.device_result(ctx, *out), em.Result(2 * w.hist, (2 * w.stats[0], 2 * w.stats[1])))
    assert not found, found


def test_without_a_stats_buffer(ctx):
    case = BY_NAME["walk_across_2000_positions_dense"]
    hist, stats = ctx.read_evidence(*em.upload(case), mbq=case.mbq, mrq=case.mrq, stats=False)
    assert stats is None
    found = em.differences(em.device_result(ctx, hist, None), case.want(), stats=False)
    assert not found, found


def test_argument_checks_and_no_ops(ctx):
    import torch

    case = BY_NAME["odd_l_seq_9"]
    bam, off, keys = em.upload(case)
    P, n = keys.numel(), off.numel()
    hist = torch.zeros((P, 4, em.METRICS, em.BINS), dtype=torch.int32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    call = ctx.lib.ampli_pileup_evidence
    INVALID = ctx.lib.ampli_pileup_indel_count(ctx.h, None, None, 0, None, 0, 20, 20, None, None, None)  # the existing "bad argument" code
    assert INVALID != 0
    good = (ctx.h, p(bam), p(off), n, p(keys), P, 20, 20, p(hist), None)
    for at, bad in ((1, None), (2, None), (3, -1), (4, None), (5, -1), (8, None)):
        args = list(good)
        args[at] = bad
        assert call(*args) == INVALID, at
        assert b"pileup_evidence: bad argument" in ctx.lib.ampli_last_error(ctx.h)
    assert call(None, *good[1:]) == INVALID
    assert call(*good[:3], 0, *good[4:]) == 0 and call(*good[:5], 0, *good[6:]) == 0  # no reads; no positions
    ctx.sync()
    assert int(hist.abs().sum()) == 0  # no refused call and no no-op counted anything
    assert call(*good) == 0
    ctx.sync()
    assert np.array_equal(hist.cpu().numpy().astype(np.int64), case.want().hist)


def device_score(ctx, planes, ref, alt):
    import torch

    up = lambda a, t: torch.from_numpy(np.ascontiguousarray(a, t)).cuda()  # noqa: E731
    ints, med, z2, used = ctx.evidence_score(up(planes, np.int32), up(ref, np.int8), up(alt, np.int8))
    ctx.sync()
    torch.cuda.synchronize()
    return em.Score(ints.cpu().numpy(), med.cpu().numpy(), z2.cpu().numpy(), used.cpu().numpy())


@pytest.mark.parametrize("name", [c[0] for c in SCORE_CASES])
def test_score_cases_integers_equal_and_z2_bit_for_bit(ctx, name):
    _, planes, ref, alt = next(c for c in SCORE_CASES if c[0] == name)
    found = em.score_differences(device_score(ctx, planes, ref, alt), em.score(planes, ref, alt))
    assert not found, found


def test_random_planes_bit_for_bit(ctx):
    planes, ref, alt = em.random_planes(np.random.default_rng(2904), 777)  # more than three workgroups of cells, the last one partial
    want = em.score(planes, ref, alt)
    assert (want.ints[:, :, 2] >= 0).sum() >= 400 and (want.z2 < 0).sum() >= 100 and (want.z2 > 0).sum() >= 100
    found = em.score_differences(device_score(ctx, planes, ref, alt), want)
    assert not found, found


def test_the_planes_the_count_kernel_wrote_scored_on_the_device(ctx):
    import torch

    case = BY_NAME[f"fuzz_{em.FUZZ_SEEDS[2]}_2500_reads_dense"]
    hist, _ = ctx.read_evidence(*em.upload(case), mbq=case.mbq, mrq=case.mrq)
    P = len(case.keys)
    rng = np.random.default_rng(2905)
    ref = rng.integers(0, 4, size=P)
    alt = np.where(rng.random(P) < 0.5, -1, (ref + 1 + rng.integers(0, 3, size=P)) % 4)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int8)).cuda()  # noqa: E731
    ints, med, z2, used = ctx.evidence_score(hist, up(ref), up(alt))
    ctx.sync()
    torch.cuda.synchronize()
    want = em.score(case.want().hist, ref, alt)
    assert (want.ints[:, :, 2] >= 0).sum() >= 100
    found = em.score_differences(em.Score(ints.cpu().numpy(), med.cpu().numpy(), z2.cpu().numpy(), used.cpu().numpy()), want)
    assert not found, found


def test_score_argument_checks(ctx):
    import torch

    hist = torch.zeros((2, 4, em.METRICS, em.BINS), dtype=torch.int32, device="cuda")
    nt = torch.zeros(2, dtype=torch.int8, device="cuda")
    ints, med = torch.zeros((2, 3, 3), dtype=torch.int64, device="cuda"), torch.zeros((2, 3, 2), dtype=torch.int32, device="cuda")
    z2, used = torch.zeros((2, 3), dtype=torch.float64, device="cuda"), torch.zeros(2, dtype=torch.int8, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    good = (ctx.h, p(hist), 2, p(nt), p(nt), p(ints), p(med), p(z2), p(used))
    call = ctx.lib.ampli_evidence_score
    for at, bad in ((1, None), (2, -1), (3, None), (4, None), (5, None), (6, None), (7, None), (8, None)):
        args = list(good)
        args[at] = bad
        assert call(*args) != 0, at
        assert b"evidence_score: bad argument" in ctx.lib.ampli_last_error(ctx.h)
    assert call(None, *good[1:]) != 0
    assert call(*good[:2], 0, *good[3:]) == 0 and call(*good) == 0
    ctx.sync()


def test_misaligned_pointers_are_refused_before_anything_is_launched(ctx):
    """ampli_pileup_evidence: d_rec_off, d_keys and d_stats below 8 bytes, d_hist below 4; ampli_evidence_score: d_int and d_z2 below 8,
    d_hist and d_med below 4.  AMPLI_E_INVALID, and the fenced outputs are untouched"""
    import torch

    from tests.helpers import assert_misaligned_refused, fenced

    case = BY_NAME["odd_l_seq_9"]
    bam, off, keys = em.upload(case)
    P = keys.numel()
    hist, stats = fenced((P, 4, em.METRICS, em.BINS), torch.int32), fenced((2,), torch.int64)
    good = (ctx.h, bam.data_ptr(), off.data_ptr(), off.numel(), keys.data_ptr(), P, 20, 20, hist[0].data_ptr(), stats[0].data_ptr())
    assert_misaligned_refused(ctx, ctx.lib.ampli_pileup_evidence, good, [(2, 4), (4, 4), (8, 2), (9, 4)], [hist, stats], b"pileup_evidence: bad argument")
    planes = torch.zeros((P, 4, em.METRICS, em.BINS), dtype=torch.int32, device="cuda")
    nt = torch.zeros(P, dtype=torch.int8, device="cuda")
    outs = [fenced((P, 3, 3), torch.int64), fenced((P, 3, 2), torch.int32), fenced((P, 3), torch.float64), fenced((P,), torch.int8)]
    good = (ctx.h, planes.data_ptr(), P, nt.data_ptr(), nt.data_ptr()) + tuple(o[0].data_ptr() for o in outs)
    assert_misaligned_refused(ctx, ctx.lib.ampli_evidence_score, good, [(1, 2), (5, 4), (6, 2), (7, 4)], outs, b"evidence_score: bad argument")
