"""The indel kernel's test model (tests/indel_model.py) checked on the CPU: its two restatements of the definition against each other on
every case, the case table against the list of deliberately wrong variants -- the evidence that tests/test_gpu_indel_kernel.py would
notice a subtly wrong kernel -- and the invariants the definition promises.  No GPU, and nothing of the product but its source text:
this file passes with or without the kernel."""
import numpy as np
import pytest

from tests import indel_model as im

CASES = im.cases()
BY_NAME = {c.name: c for c in CASES}


def _same(a, b):
    return np.array_equal(a.counts, b.counts) and np.array_equal(a.lengths, b.lengths) and tuple(a.stats) == tuple(b.stats)


def test_the_geometry_is_read_from_the_sources():
    geo = im.geometry()
    assert geo.reads >= 64 and geo.window >= 64 and geo.bins == im.BINS == 32
    text = open(im.KERNEL_SOURCE).read()
    assert "win[INDEL_WINDOW * 2]" in text and "wkeys[INDEL_WINDOW]" in text and "blockIdx.x * INDEL_READS" in text
    assert len({c.name for c in CASES}) == len(CASES)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_the_two_restatements_agree(case):
    a, b = case.want(), im.walk(case.stream, case.keys, case.mbq, case.mrq)
    assert _same(a, b), (a.stats, b.stats, np.argwhere(a.counts != b.counts)[:5].tolist())


@pytest.mark.parametrize("variant", sorted(im.WRONG_VARIANTS))
def test_every_wrong_variant_is_caught_by_its_named_cases(variant):
    assert set(im.CAUGHT_BY) == set(im.WRONG_VARIANTS)
    for name in im.CAUGHT_BY[variant]:
        case = BY_NAME[name]
        assert not _same(case.want(), case.want(wrong=variant)), f"{variant} ({im.WRONG_VARIANTS[variant]}) passes {name}"


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_invariants(case):
    w = case.want()
    assert not w.counts[:, 3].any() and not w.counts[:, 7].any()                              # T is never written
    assert np.array_equal(w.lengths.sum(2), w.counts[:, 1:3])                                 # the bins of a kind sum to its slot
    assert np.all(w.counts[:, 4:7] <= w.counts[:, 0:3]) and w.counts.min() >= 0               # the reverse strand is part of the total
    assert w.stats[1] == w.counts[:, :3].sum() and w.stats[0] <= case.n_reads
    assert np.all(w.counts[:, :3].sum(1) <= im.covering(case.stream, case.keys, case.mrq))    # A + C + G <= the reads covering p


def test_the_fuzz_streams_hold_what_the_issue_asks_for():
    """re-counted here so that a failure names the figures (the table's own asserts already hold them)"""
    import collections

    tally = collections.Counter()
    ins = dele = 0
    for c in im.fuzz_cases():
        assert c.n_reads <= 3000
        got = im.walk(c.stream, c.keys, c.mbq, c.mrq, tally)
        ins, dele = ins + int(got.counts[:, 1].sum()), dele + int(got.counts[:, 2].sum())
    print(f"insertions {ins}, deletions {dele}, " + ", ".join(f"{k} {tally[k]}" for k in im.REJECTIONS + ("events_reverse",)))
    assert ins >= 50 and dele >= 50 and all(tally[k] >= 10 for k in im.REJECTIONS) and tally["events_reverse"] >= 10


def test_the_model_streams_pass_the_products_record_scanner(tmp_path):
    """ampli_host_bam_scan on the records of the fuzz cases as BAM files: all listed, none malformed -- what computeIndelCounts will count"""
    import ctypes as C

    from amplisolve_amd import host_lib

    lib = host_lib()
    for k, case in enumerate(im.fuzz_cases()):
        path = tmp_path / f"f{k}.bam"
        im.write_bam_of(str(path), case.buf, case.rec_off)
        stats = (C.c_int64 * 4)()
        assert lib.ampli_host_bam_scan(str(path).encode(), 2, stats) == 0
        assert (stats[0], stats[3]) == (case.n_reads, 0)
