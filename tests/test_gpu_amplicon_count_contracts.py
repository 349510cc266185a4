"""What ampli_pileup_amplicon_count and ampli_amplicon_layers write, on poisoned and fenced buffers (helpers.fenced): the count call ADDS
to the counters it owns inside [0, W) and [0, A) and touches nothing else, with and without the optional statistics; the layers call
OVERWRITES every cell of its three outputs and nothing beyond them (contracts C29 and C30 of include/amplisolve_hip.h)."""
import numpy as np
import pytest

from tests import amplicon_count_model as am
from tests import helpers

pytestmark = pytest.mark.gpu
BY_NAME = {c.name: c for c in am.cases()}
NAMES = ["fuzz_28002_1777_reads", "reads_straddle_the_windows_first_and_last_entry", "read_assigned_outside_the_window_unsorted_stream",
         "65_amplicons_shifted_by_one_second_round_of_lanes", "amplicon_of_length_1"]


@pytest.fixture(scope="module")
def ctx():
    from amplisolve_amd.api import Context

    c = Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("with_stats", [True, False])
@pytest.mark.parametrize("name", NAMES)
def test_the_count_call_adds_inside_its_extents_and_writes_nothing_else(ctx, name, with_stats):
    import torch

    case = BY_NAME[name]
    A, W = len(case.amps.lo), int(case.amps.amp_off[-1])
    counts, check_counts = helpers.fenced((W, 8), torch.int32)
    amp_reads, check_reads = helpers.fenced((A, 2), torch.int64)
    stats, check_stats = helpers.fenced((4,), torch.int64)
    counts.fill_(1000)  # what the call adds to: poison is for what it must not touch
    amp_reads.fill_(2000)
    stats.fill_(3000)
    ctx.amplicon_count(*am.upload(case), mbq=case.mbq, mrq=case.mrq, min_overlap=case.min_overlap, counts=counts, amp_reads=amp_reads,
                       stats=stats if with_stats else False)
    got = am.host(ctx, counts, amp_reads, stats)
    want = case.want()
    assert np.array_equal(got[0] - 1000, want.counts) and np.array_equal(got[1] - 2000, want.amp_reads)
    assert (got[2] - 3000).tolist() == (list(want.stats) if with_stats else [0, 0, 0, 0])
    check_counts()
    check_reads()
    check_stats()


@pytest.mark.parametrize("L", [0, 1, 2, 4])
@pytest.mark.parametrize("name", NAMES[:2] + ["three_amplicons_over_one_position_L_2"])
def test_the_layers_call_overwrites_every_cell_and_nothing_beyond(ctx, name, L):
    import torch

    case = BY_NAME[name]
    amps = am.upload_amplicons(case)
    counts, _, _ = ctx.amplicon_count(*am.upload(case), mbq=case.mbq, mrq=case.mrq, min_overlap=case.min_overlap)
    keys = np.concatenate([case.keys[::-1], case.keys[:37], np.asarray([am.key_of(9, 5)], np.uint64)])  # 2 mod 256 and more than one block where the case is large
    P = len(keys)
    outs = [helpers.fenced(shape, torch.int32, poison=poison) for shape, poison in (((max(L, 1), P, 8), 0xFF), ((max(L, 1), P), 0x5A), ((P, 8), 0xFF))]
    (layers, c0), (layer_amp, c1), (total, c2) = outs
    ctx.amplicon_layers(counts, *amps, am._up(keys), L=L, layers=layers[:L], layer_amp=layer_amp[:L], total=total)
    got = am.host(ctx, layers[:L], layer_amp[:L], total)
    want = am.layers(case.want().counts, case.amps, keys, L)
    assert np.array_equal(got[0], want.layers) and np.array_equal(got[1], want.layer_amp) and np.array_equal(got[2], want.total)
    if L == 0:  # the row that L = 0 leaves alone still holds the poison
        assert bool((layers.view(torch.uint8) == 0xFF).all()) and bool((layer_amp.view(torch.uint8) == 0x5A).all())
    for c in (c0, c1, c2):
        c()


def test_misaligned_pointers_are_refused_before_anything_is_launched(ctx):
    """ampli_pileup_amplicon_count: every 8-byte array below 8 bytes, d_counts below 4.  ampli_amplicon_layers: d_counts, d_layers and
    d_total below 16 bytes (the gather loads and stores int4), the 8-byte arrays below 8, d_layer_amp below 4.  AMPLI_E_INVALID, and the
    fenced outputs (the statistics included) are untouched"""
    import torch

    case = BY_NAME["three_amplicons_over_one_position_L_2"]
    bam, off, lo, hi, reach, amp_off = am.upload(case)
    A, W = len(case.amps.lo), int(case.amps.amp_off[-1])
    counts, amp_reads, stats = helpers.fenced((W, 8), torch.int32), helpers.fenced((A, 2), torch.int64), helpers.fenced((4,), torch.int64)
    ptr = lambda t: t.data_ptr()  # noqa: E731
    good = (ctx.h, ptr(bam), ptr(off), off.numel(), ptr(lo), ptr(hi), ptr(reach), ptr(amp_off), A, W, case.mbq, case.mrq, case.min_overlap, ptr(counts[0]),
            ptr(amp_reads[0]), ptr(stats[0]))
    helpers.assert_misaligned_refused(ctx, ctx.lib.ampli_pileup_amplicon_count, good, [(2, 4), (4, 4), (5, 4), (6, 4), (7, 4), (13, 2), (14, 4), (15, 4)],
                                      [counts, amp_reads, stats], b"pileup_amplicon_count: bad argument")
    walked = torch.zeros((W, 8), dtype=torch.int32, device="cuda")
    keys = am._up(case.keys)
    P = keys.numel()
    layers, layer_amp, total = helpers.fenced((2, P, 8), torch.int32), helpers.fenced((2, P), torch.int32), helpers.fenced((P, 8), torch.int32)
    good = (ctx.h, ptr(walked), ptr(lo), ptr(hi), ptr(reach), ptr(amp_off), A, W, ptr(keys), P, 2, ptr(layers[0]), ptr(layer_amp[0]), ptr(total[0]))
    helpers.assert_misaligned_refused(ctx, ctx.lib.ampli_amplicon_layers, good, [(1, 4), (1, 8), (2, 4), (3, 4), (4, 4), (5, 4), (8, 4), (11, 4), (11, 8), (12, 2), (13, 4), (13, 8)],
                                      [layers, layer_amp, total], b"amplicon_layers: bad argument")
