"""ampli_pileup_amplicon_count and ampli_amplicon_layers themselves (through Context.amplicon_count / .amplicon_layers), one call per case
of the table of tests/amplicon_count_model.py, against the model: every integer of counts, amp_reads, stats, the layers and the totals."""
import ctypes as C

import numpy as np
import pytest

from tests import amplicon_count_model as am

pytestmark = pytest.mark.gpu
CASES = am.cases()
BY_NAME = {c.name: c for c in CASES}


@pytest.fixture(scope="module")
def ctx():
    from amplisolve_amd.api import Context

    c = Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_every_integer_equals_the_models(ctx, case):
    amps = am.upload_amplicons(case)
    counts, amp_reads, stats = ctx.amplicon_count(*am.upload(case), mbq=case.mbq, mrq=case.mrq, min_overlap=case.min_overlap)
    layers, layer_amp, total = ctx.amplicon_layers(counts, *amps, am._up(case.keys), L=case.L)
    got = am.host(ctx, counts, amp_reads, stats, layers, layer_amp, total)
    assert am.differences(*got[:3], case.want()) == []
    want = case.want_layers()
    assert np.array_equal(got[3], want.layers) and np.array_equal(got[4], want.layer_amp) and np.array_equal(got[5], want.total)


@pytest.mark.parametrize("name", ["fuzz_28001_3000_reads", "fuzz_28002_1777_reads", "one_read_more_than_a_read_group", "reads_straddle_the_windows_first_and_last_entry"])
def test_a_stream_counted_in_two_halves_accumulates_to_the_whole(ctx, name):
    case = BY_NAME[name]
    half = case.n_reads // 2 + 1
    kw = dict(mbq=case.mbq, mrq=case.mrq, min_overlap=case.min_overlap)
    out = ctx.amplicon_count(*am.upload(case, 0, half), **kw)
    out = ctx.amplicon_count(*am.upload(case, half, None), **kw, counts=out[0], amp_reads=out[1], stats=out[2])
    assert am.differences(*am.host(ctx, *out), case.want()) == []


def test_without_the_statistics_and_other_thresholds(ctx):
    case = BY_NAME["fuzz_28003_2500_reads"]
    for min_overlap in (1, 50, 100):
        counts, amp_reads, stats = ctx.amplicon_count(*am.upload(case), mbq=case.mbq, mrq=case.mrq, min_overlap=min_overlap, stats=False)
        assert stats is None
        want = am.count(case.stream, case.amps, case.mbq, case.mrq, min_overlap)
        assert am.differences(*am.host(ctx, counts, amp_reads), None, want) == []


def test_layers_of_one_three_and_no_layer_and_keys_in_any_order(ctx):
    case = BY_NAME["three_amplicons_over_one_position_L_2"]
    amps = am.upload_amplicons(case)
    counts, _, _ = ctx.amplicon_count(*am.upload(case))
    rng = np.random.default_rng(4)
    keys = np.concatenate([case.keys, case.keys[::5], np.asarray([am.key_of(0, 1), am.key_of(1, 1095), am.key_of(0, 2 ** 31 - 1)], np.uint64)])
    keys = keys[rng.permutation(len(keys))]
    for L in (0, 1, 3):
        got = am.host(ctx, *ctx.amplicon_layers(counts, *amps, am._up(keys), L=L))
        want = am.layers(case.want().counts, case.amps, keys, L)
        assert np.array_equal(got[0], want.layers) and np.array_equal(got[1], want.layer_amp) and np.array_equal(got[2], want.total)


def test_the_argument_checks_and_no_ops(ctx):
    import torch

    case = BY_NAME["read_equals_its_amplicon_A_is_1"]
    bam, off, lo, hi, reach, amp_off = am.upload(case)
    W = 100
    counts = torch.full((W, 8), 7, dtype=torch.int32, device="cuda")
    amp_reads = torch.full((1, 2), 7, dtype=torch.int64, device="cuda")
    stats = torch.full((4,), 7, dtype=torch.int64, device="cuda")
    keys = am._up(case.keys)
    P = keys.numel()
    layers = torch.full((2, P, 8), 7, dtype=torch.int32, device="cuda")
    layer_amp = torch.full((2, P), 7, dtype=torch.int32, device="cuda")
    total = torch.full((P, 8), 7, dtype=torch.int32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)  # noqa: E731
    call, gather = ctx.lib.ampli_pileup_amplicon_count, ctx.lib.ampli_amplicon_layers

    def count_args(n=1, A=1, W_=W, min_overlap=50, **null):
        t = dict(bam=bam, off=off, lo=lo, hi=hi, reach=reach, amp_off=amp_off, counts=counts, amp_reads=amp_reads, stats=stats)
        t.update(null)
        return (ctx.h, p(t["bam"]), p(t["off"]), n, p(t["lo"]), p(t["hi"]), p(t["reach"]), p(t["amp_off"]), A, W_, 20, 20, min_overlap, p(t["counts"]), p(t["amp_reads"]),
                p(t["stats"]))

    def layer_args(A=1, W_=W, P_=P, L=2, **null):
        t = dict(counts=counts, lo=lo, hi=hi, reach=reach, amp_off=amp_off, keys=keys, layers=layers, layer_amp=layer_amp, total=total)
        t.update(null)
        return (ctx.h, p(t["counts"]), p(t["lo"]), p(t["hi"]), p(t["reach"]), p(t["amp_off"]), A, W_, p(t["keys"]), P_, L, p(t["layers"]), p(t["layer_amp"]), p(t["total"]))

    INVALID, RANGE = -1, -6  # AMPLI_E_INVALID, AMPLI_E_RANGE of include/amplisolve_hip.h
    for name in ("bam", "off", "lo", "hi", "reach", "amp_off", "counts", "amp_reads"):
        assert call(*count_args(**{name: None})) == INVALID, name
        assert b"pileup_amplicon_count: bad argument" in ctx.lib.ampli_last_error(ctx.h)
    for kw in (dict(n=-1), dict(A=-1), dict(W_=-1), dict(min_overlap=0), dict(min_overlap=101), dict(min_overlap=-50)):
        assert call(*count_args(**kw)) == INVALID, kw
    assert call(*count_args(W_=2 ** 31)) == RANGE and call(*count_args(n=am.geometry().reads * (2 ** 31 - 1) + 1)) == RANGE
    for name in ("counts", "lo", "hi", "reach", "amp_off", "keys", "layers", "layer_amp", "total"):
        assert gather(*layer_args(**{name: None})) == INVALID, name
        assert b"amplicon_layers: bad argument" in ctx.lib.ampli_last_error(ctx.h)
    for kw in (dict(A=-1), dict(W_=-1), dict(P_=-1), dict(L=-1)):
        assert gather(*layer_args(**kw)) == INVALID, kw
    assert gather(*layer_args(W_=2 ** 31)) == RANGE
    # the no-ops: A = 0, n_reads = 0, P = 0 succeed and write nothing
    assert call(*count_args(n=0)) == 0 and call(*count_args(A=0, W_=0)) == 0 and gather(*layer_args(P_=0)) == 0 and gather(*layer_args(A=0, W_=0)) == 0
    ctx.sync()
    for t in (counts, amp_reads, stats, layers, layer_amp, total):
        assert bool((t == 7).all())
    # and the same call with nothing withheld counts
    assert call(*count_args(stats=None)) == 0 and gather(*layer_args()) == 0
    ctx.sync()
    assert int(counts.sum()) == 7 * W * 8 + 100 and amp_reads.tolist() == [[8, 7]] and bool((stats == 7).all()) and int(layer_amp[0].max()) == 0
