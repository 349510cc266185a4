"""The amplicon counting kernels' test model (tests/amplicon_count_model.py) checked on the CPU: its two restatements of the definition
against each other on every case, the case table against the list of deliberately wrong variants -- the evidence that
tests/test_gpu_amplicon_count_kernel.py would notice such a kernel -- and the invariants that tie the counts, the layers, the totals and
the pooled pileup together.  Needs the kernel's source text (its geometry), not the build."""
import numpy as np
import pytest

from tests import amplicon_count_model as am
from tests import pileup_model as pm

CASES = am.cases()
BY_NAME = {c.name: c for c in CASES}


def test_the_geometry_is_read_from_the_kernel_source():
    geo = am.geometry()
    text = open(am.KERNEL_SOURCE).read()
    assert geo.reads >= 64 and geo.window >= 64
    assert "win[AMPCOUNT_WINDOW * 8]" in text and "blockIdx.x * AMPCOUNT_READS" in text
    assert len(CASES) == len(BY_NAME) and max(c.n_reads for c in CASES) > 4 * geo.reads


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_the_two_restatements_agree(case):
    want = case.want()
    counts, amp_reads, stats = am.walk(case.stream, case.amps, case.mbq, case.mrq, case.min_overlap)
    assert am.differences(counts, amp_reads, stats, want) == []
    assert int(want.counts[:, :4].sum()) == want.stats[2]  # the sum of counts is bases_counted
    assert int(want.amp_reads.sum()) == want.stats[1] <= want.stats[0]
    assert int(want.n_clipped.sum()) == want.stats[3]


@pytest.mark.parametrize("variant", sorted(am.WRONG_VARIANTS))
def test_every_wrong_variant_is_caught_by_its_named_cases(variant):
    assert set(am.CAUGHT_BY) == set(am.WRONG_VARIANTS)
    for name in am.CAUGHT_BY[variant]:
        case = BY_NAME[name]
        if variant == "total_drops_beyond_L":
            got, want = case.want_layers(wrong=variant), case.want_layers()
            assert not np.array_equal(got.total, want.total), name
            assert np.array_equal(got.layers, want.layers) and np.array_equal(got.layer_amp, want.layer_amp)
        else:
            got, want = case.want(wrong=variant), case.want()
            assert am.differences(got.counts, got.amp_reads, got.stats, want) != [], (variant, name)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_layers_totals_and_the_pooled_pileup(case):
    """the sum over the layers is <= the totals, and the totals are <= the pooled pileup of the same stream, cell by cell: the amplicon
    walk drops clipped columns and off-target reads and adds nothing"""
    lay = case.want_layers()
    present = lay.layer_amp >= 0
    assert np.all((lay.layers[:, :, 0] == am.ABSENT) == ~present) and np.all(lay.layers[~present][:, 1:] == 0)
    layer_sum = np.where(present[:, :, None], lay.layers, 0).sum(0)
    assert np.all(layer_sum <= lay.total)
    n_cover = np.asarray([len(am.covering(case.amps, k)) for k in case.keys.tolist()])
    assert np.array_equal(layer_sum[n_cover <= case.L], lay.total[n_cover <= case.L]) and np.all(lay.total[n_cover == 0] == 0)
    keys, inverse = np.unique(case.keys, return_inverse=True)
    pooled = pm.count(case.stream, keys, case.mbq, case.mrq)[0][inverse]
    assert np.all(lay.total <= pooled)
    if case.want().stats[3] == 0 and case.want().stats[0] == case.want().stats[1] and len(keys) == len(case.keys):
        # nothing clipped, nothing off-target: the totals over all positions of all amplicons hold every counted base
        assert int(lay.total[:, :4].sum()) == case.want().stats[2]


def test_the_gather_takes_keys_in_any_order_and_repeated():
    case = BY_NAME["three_amplicons_over_one_position_L_2"]
    rng = np.random.default_rng(3)
    keys = np.concatenate([case.keys, case.keys[::7]])[rng.permutation(len(case.keys) + len(case.keys[::7]))]
    got = am.layers(case.want().counts, case.amps, keys, 3)
    at = np.searchsorted(case.keys, keys)
    assert np.array_equal(got.total, case.want_layers().total[at]) and np.array_equal(got.layers[:2], case.want_layers().layers[:, at])
    assert (got.layer_amp[2] >= 0).sum() > 0
