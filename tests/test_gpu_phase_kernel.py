"""ampli_pileup_phase and ampli_phase_score themselves (through amplisolve_amd.read_phase / phase_score), one call per case of the table of
tests/phase_model.py, against the model: exact integer equality of every cell and of the stats; halves of a stream that accumulate to the
whole; the argument checks and no-ops; the invariant on the device's own table; the score kernel on the model's tables, integers and
classes equal and scores within S_TOL."""
import ctypes as C
import time

import numpy as np
import pytest

from tests import phase_model as ph

pytestmark = pytest.mark.gpu
CASES = ph.cases()
BY_NAME = {c.name: c for c in CASES}
SCORE_CASES = ph.score_cases()
SHAPE = (ph.K, ph.STATES, ph.STATES)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_cells_and_stats_equal_the_model(ctx, case):
    from amplisolve_amd import read_phase

    t0 = time.perf_counter()
    got = ph.device_result(ctx, *read_phase(ctx, *ph.upload(case), mbq=case.mbq, mrq=case.mrq))
    want = case.want()
    print(f"{case!r}: {time.perf_counter() - t0:.3f} s incl. upload and model; stats {got.stats}")
    found = ph.differences(got, want)
    assert not found, found


@pytest.mark.parametrize("name", ["a_stream_in_descending_position_order_dense", "a_stream_in_ascending_position_order_sparse", "257_reads",
                                  f"fuzz_{ph.FUZZ_SEEDS[0]}_900_reads_sparse", f"fuzz_{ph.FUZZ_SEEDS[1]}_777_reads_dense"])
def test_two_calls_on_halves_accumulate_to_the_whole(ctx, name):
    from amplisolve_amd import read_phase

    case = BY_NAME[name]
    half = case.n_reads // 2 + 1
    out = read_phase(ctx, *ph.upload(case, 0, half), mbq=case.mbq, mrq=case.mrq)
    out = read_phase(ctx, *ph.upload(case, half, None), mbq=case.mbq, mrq=case.mrq, table=out[0], stats=out[1])
    found = ph.differences(ph.device_result(ctx, *out), case.want())
    assert case.want().stats[2] > 0 and not found, found


def test_without_a_stats_buffer(ctx):
    from amplisolve_amd import read_phase

    case = BY_NAME["a_stream_in_descending_position_order_dense"]
    table, stats = read_phase(ctx, *ph.upload(case), mbq=case.mbq, mrq=case.mrq, stats=False)
    assert stats is None
    found = ph.differences(ph.device_result(ctx, table, None), case.want(), stats=False)
    assert not found, found


def test_the_invariant_on_the_devices_table(ctx):
    from amplisolve_amd import read_phase

    for name in (f"fuzz_{ph.FUZZ_SEEDS[0]}_900_reads_sparse", "nine_keys_inside_one_read"):
        case = BY_NAME[name]
        got = ph.device_result(ctx, *read_phase(ctx, *ph.upload(case), mbq=case.mbq, mrq=case.mrq))
        assert len(case.invariant_cells()) >= ph.INVARIANT_CASES[name]
        bad = ph.invariant_failures(case, got.table)
        assert not bad, bad[:3]


def test_argument_checks_and_no_ops(ctx):
    import torch

    case = BY_NAME["leading_5S"]
    bam, off, keys = ph.upload(case)
    P, n = keys.numel(), off.numel()
    table = torch.zeros((P,) + SHAPE, dtype=torch.int32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    call = ctx.lib.ampli_pileup_phase
    good = (p(bam), p(off), n, p(keys), P, 20, 20, p(table), None, ctx.h)
    for at, bad in ((0, None), (1, None), (2, -1), (3, None), (4, -1), (7, None)):
        args = list(good)
        args[at] = bad
        assert call(*args) == -1, at
        assert b"pileup_phase: bad argument" in ctx.lib.ampli_last_error(ctx.h)
    assert call(*good[:-1], None) == -1
    assert call(*good[:2], 0, *good[3:]) == 0 and call(*good[:4], 0, *good[5:]) == 0  # no reads; no positions
    ctx.sync()
    assert int(table.abs().sum()) == 0  # no refused call and no no-op counted anything
    assert call(*good) == 0
    ctx.sync()
    assert np.array_equal(table.cpu().numpy().astype(np.int64), case.want().table)


def device_score(ctx, table, cells, nts, min_alt=4, min_share=10):
    import torch

    from amplisolve_amd import phase_score

    up = lambda a, t: torch.from_numpy(np.ascontiguousarray(a, t)).cuda()  # noqa: E731
    ints, score, cls = phase_score(ctx, up(np.asarray(table).reshape((-1,) + SHAPE), np.int32), up(cells, np.int64), up(np.asarray(nts).reshape(-1, 4), np.int8), min_alt, min_share)
    ctx.sync()
    torch.cuda.synchronize()
    return ph.Score(ints.cpu().numpy(), score.cpu().numpy(), cls.cpu().numpy(), None)


@pytest.mark.parametrize("name", [c[0] for c in SCORE_CASES])
def test_score_cases_integers_and_classes_equal_scores_within_s_tol(ctx, name):
    _, table, cells, nts, min_alt, min_share = next(c for c in SCORE_CASES if c[0] == name)
    found = ph.score_differences(device_score(ctx, table, cells, nts, min_alt, min_share), ph.score(table, cells, nts, min_alt, min_share))
    assert not found, found


def test_random_tables(ctx):
    t, cells, nts = ph.random_tables(np.random.default_rng(3204), 70)  # more than two workgroups of pairs, the last one partial
    assert len(cells) > 512
    for min_alt, min_share in ((4, 10), (1, 0)):
        found = ph.score_differences(device_score(ctx, t, cells, nts, min_alt, min_share), ph.score(t, cells, nts, min_alt, min_share))
        assert not found, found


def test_the_table_the_count_kernel_wrote_scored_on_the_device(ctx):
    import torch

    from amplisolve_amd import phase_score, read_phase

    case = BY_NAME[f"fuzz_{ph.FUZZ_SEEDS[2]}_600_reads_dense"]
    table, _ = read_phase(ctx, *ph.upload(case), mbq=case.mbq, mrq=case.mrq)
    rng = np.random.default_rng(3205)
    Q = 600
    cells = rng.integers(0, len(case.keys) * ph.K, size=Q)
    ref = rng.integers(0, 4, size=(Q, 2))
    alt = (ref + 1 + rng.integers(0, 3, size=(Q, 2))) % 4
    nts = np.stack([ref[:, 0], alt[:, 0], ref[:, 1], alt[:, 1]], 1)
    want = ph.score(case.want().table, cells, nts, 1, 0)
    assert (want.cls > 0).sum() >= 20 and (want.score != 0).sum() >= 20
    ints, score, cls = phase_score(ctx, table, torch.from_numpy(cells).cuda(), torch.from_numpy(nts.astype(np.int8)).cuda(), 1, 0)
    ctx.sync()
    torch.cuda.synchronize()
    found = ph.score_differences(ph.Score(ints.cpu().numpy(), score.cpu().numpy(), cls.cpu().numpy(), None), want)
    assert not found, found


def test_score_argument_checks(ctx):
    import torch

    table = torch.zeros((2,) + SHAPE, dtype=torch.int32, device="cuda")
    cells, nts = torch.zeros(2, dtype=torch.int64, device="cuda"), torch.zeros((2, 4), dtype=torch.int8, device="cuda")
    ints, score, cls = torch.zeros((2, 6), dtype=torch.int64, device="cuda"), torch.zeros(2, dtype=torch.float32, device="cuda"), torch.zeros(2, dtype=torch.int32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    good = (p(table), 2, p(cells), p(nts), 2, 4, 10, p(ints), p(score), p(cls), ctx.h)
    call = ctx.lib.ampli_phase_score
    for at, bad in ((0, None), (1, -1), (2, None), (3, None), (4, -1), (5, 0), (6, -1), (6, 101), (7, None), (8, None), (9, None)):
        args = list(good)
        args[at] = bad
        assert call(*args) == -1, at
        assert b"phase_score: bad argument" in ctx.lib.ampli_last_error(ctx.h)
    assert call(*good[:-1], None) == -1
    assert call(*good[:4], 0, *good[5:]) == 0 and call(*good) == 0
    ctx.sync()


def test_misaligned_pointers_are_refused_before_anything_is_launched(ctx):
    """ampli_pileup_phase: d_rec_off, d_keys and d_stats below 8 bytes, d_table below 4; ampli_phase_score: d_pair_cell and d_int below 8,
    d_table, d_score and d_class below 4.  AMPLI_E_INVALID, and the fenced outputs are untouched"""
    import torch

    from tests.helpers import fenced

    def refused(call, good, shifts, outputs, message):  # tests/helpers.assert_misaligned_refused for entry points whose context comes last
        for at, by in shifts:
            args = list(good)
            assert isinstance(args[at], int) and args[at] % 16 == 0 and 0 < by < 16, at
            args[at] += by
            assert call(*args) == -1, f"argument {at} moved by {by} byte(s) was not refused"
            assert message in ctx.lib.ampli_last_error(ctx.h), ctx.lib.ampli_last_error(ctx.h)
        ctx.sync()
        torch.cuda.synchronize()
        for view, check in outputs:
            assert bool((check.raw == check.raw[0]).all()), "a refused call wrote to an output"
            check()

    case = BY_NAME["leading_5S"]
    bam, off, keys = ph.upload(case)
    P = keys.numel()
    table, stats = fenced((P,) + SHAPE, torch.int32), fenced((3,), torch.int64)
    good = (bam.data_ptr(), off.data_ptr(), off.numel(), keys.data_ptr(), P, 20, 20, table[0].data_ptr(), stats[0].data_ptr(), ctx.h)
    refused(ctx.lib.ampli_pileup_phase, good, [(1, 4), (3, 4), (7, 2), (8, 4)], [table, stats], b"pileup_phase: bad argument")
    t = torch.zeros((P,) + SHAPE, dtype=torch.int32, device="cuda")
    cells, nts = torch.zeros(4, dtype=torch.int64, device="cuda"), torch.zeros((4, 4), dtype=torch.int8, device="cuda")
    outs = [fenced((4, 6), torch.int64), fenced((4,), torch.float32), fenced((4,), torch.int32)]
    good = (t.data_ptr(), P, cells.data_ptr(), nts.data_ptr(), 4, 4, 10) + tuple(o[0].data_ptr() for o in outs) + (ctx.h,)
    refused(ctx.lib.ampli_phase_score, good, [(0, 2), (2, 4), (7, 4), (8, 2), (9, 2)], outs, b"phase_score: bad argument")
