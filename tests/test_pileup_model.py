"""The pileup kernel's test model (tests/pileup_model.py) checked on the CPU: its vectorised reference against the per-base Python
restatement (oracle/pileup_oracle.py) through a real BAM file, its streams against the product's own record scanner, and the case
table against a list of deliberately wrong references -- the evidence that tests/test_gpu_pileup_kernel.py would notice a subtly
wrong kernel."""
import ctypes as C

import numpy as np
import pytest

from amplisolve_amd import host_lib
from oracle import pileup_oracle as po
from tests import pileup_model as pm

ORACLE_MAX_BASES = 400_000  # the Python loop takes about a microsecond per query base and key lookup


class _RefNames:
    """pileup_oracle.pileup names chromosomes through refs[ref_id]: here the name of a reference is its id"""

    def __getitem__(self, ref_id):
        return ref_id


def _oracle_counts(case, tmp_path, max_reads=None):
    """counts [P][8] of the case by pileup_oracle, from the builder's bytes wrapped into a BAM file and read back"""
    buf, off = case.stream
    if max_reads is not None:
        off = off[:max_reads]
    path = tmp_path / "case.bam"
    pm.write_bam_of(path, buf, off)
    _, recs = po.read_bam(path)
    assert len(recs) == len(off)
    positions = [(int(k) >> 32, int(k) & 0xffffffff) for k in case.keys]
    got = po.pileup(_RefNames(), recs, positions, case.mbq, case.mrq)
    return np.asarray([got[p] for p in positions], np.int64), recs, (buf, off)


def _small(case):
    return int(pm.headers(*case.stream).l_seq.sum()) <= ORACLE_MAX_BASES


def test_geometry_is_read_from_the_kernel_source():
    g = pm.geometry()
    text = open(pm.KERNEL_SOURCE).read()
    assert "stage[PILEUP_STAGE + 32]" in text and "win[PILEUP_SWINDOW * 8]" in text and "blockIdx.x * PILEUP_READS" in text
    assert g.reads > 0 and g.stage % 16 == 0 and g.window > 0
    assert g.reads == 256  # both kernels are launched with 256 threads and walk one read per thread of a group


def test_the_builder_round_trips_through_the_oracles_reader(tmp_path):
    rng = np.random.default_rng(3)
    reads = [pm.read(2, 77, "3H2S10M1I4M2D3M5N6=1X1P2S", rng, flag=0x91, mapq=17, name="n" * 254), pm.read(0, 0, "1M", rng, name=""),
             pm.read(-1, -1, "", rng), pm.read(5, 9, "33M", rng, seq=pm.SEQ_CODE * 2 + "A", qual=list(range(223, 256)))]
    buf, off = pm.build_stream(reads, lead=13, gaps={1: 5, 3: 40}, trail=21)
    assert int(off[0]) == 13 and len(buf) - int(pm.headers(buf, off).end[-1]) == 21
    filler = np.ones(len(buf), bool)
    h = pm.headers(buf, off)
    for a, b in zip(h.off, h.end):
        filler[a:b] = False
    assert filler.sum() == 13 + 5 + 40 + 21 and np.all(buf[filler] != 0)
    pm.write_bam_of(tmp_path / "b.bam", buf, off)
    _, recs = po.read_bam(tmp_path / "b.bam")
    assert [{k: r[k] for k in ("ref_id", "pos", "mapq", "flag", "cigar", "seq", "qual")} for r in reads] == recs
    assert h.l_name.tolist() == [255, 1, 3, 3]


@pytest.mark.parametrize("lead", list(range(16)) + [16, 37])
def test_the_first_record_takes_every_phase(lead):
    rng = np.random.default_rng(lead)
    buf, off = pm.build_stream([pm.read(0, 999, "20M", rng), pm.read(0, 999, "21M", rng)], lead=lead)
    assert int(off[0]) % 16 == lead % 16
    assert pm.group_spans(buf, off).tolist() == [[lead & ~15, int(pm.headers(buf, off).end[-1])]]
    assert pm.count((buf, off), pm.span_keys(0, 1000, 1030), 0, 0)[2] == 41


def test_every_deterministic_case_equals_the_python_oracle(tmp_path):
    checked = 0
    for case in pm.deterministic_cases():
        if not _small(case):
            continue
        want, recs, _ = _oracle_counts(case, tmp_path)
        got, kept, added = case.want()
        assert np.array_equal(got, want), case.name
        assert kept == sum(1 for r in recs if r["ref_id"] >= 0 and r["pos"] >= 0 and not r["flag"] & 0x704 and r["mapq"] >= case.mrq), case.name
        assert added == int(want[:, :4].sum()), case.name
        checked += 1
    assert checked >= len(pm.deterministic_cases()) - 2  # all but the 100 000-base read and the longest walk fit the Python loop


def test_fuzz_streams_equal_the_python_oracle(tmp_path):
    cases = pm.fuzz_cases(max_reads=1500)
    assert len(cases) >= 20
    for case in cases:
        want, _, stream = _oracle_counts(case, tmp_path)
        got, _, added = pm.count(stream, case.keys, case.mbq, case.mrq)
        assert np.array_equal(got, want), case.name
        assert added == int(want[:, :4].sum()), case.name


def test_the_counted_bases_add_up_to_the_counts():
    for case in pm.deterministic_cases()[:40]:
        counts, _, added, d = case.want(detail=True)
        assert len(d.read) == len(d.key) == added
        assert np.array_equal(np.bincount(d.key, minlength=len(case.keys)), counts[:, :4].sum(1)), case.name


def test_the_table_covers_what_it_claims():
    """the claims that need the whole table (each single case asserts its own while it is built)"""
    g = pm.geometry()
    det = {c.name: c for c in pm.deterministic_cases()}
    assert {f"group_size_{n}" for n in (1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1025)} <= set(det)
    assert sum(n.startswith("stage_") for n in det) == 15
    names = [c.name for c in pm.cases()]
    assert len(names) == len(set(names))
    fuzz = [c for c in pm.cases() if c.name.startswith("fuzz_")]
    assert len(fuzz) >= 20 and min(c.n_reads for c in fuzz) == 1 and max(c.n_reads for c in fuzz) >= 50_000
    assert all(len(c.keys) > 2 * g.window for c in fuzz)
    assert any(c.staged().all() for c in fuzz) and any((~c.staged()).any() and c.staged().any() for c in fuzz)
    assert {int(c.rec_off[0]) % 16 for c in fuzz} >= set(range(0, 16, 5))
    depth = [c for c in pm.cases() if c.name.startswith("depth_")]
    assert len(depth) == 1 and depth[0].n_reads == pm.DEPTH_READS and len(depth[0].keys) == 120


def test_the_host_scanner_accepts_every_record_of_every_case(tmp_path):
    """ampli_host_bam_scan on the records of each case as a BAM file: all of them listed, none malformed -- so the kernel tests
    never hand the device a record the product would have dropped.  (The file holds the listed records without the filler between
    them: the filler stands for records the scanner HAS dropped.)"""
    lib = host_lib()
    for case in pm.cases():
        path = tmp_path / "s.bam"
        pm.write_bam_of(path, *case.stream)
        stats = (C.c_int64 * 4)()
        rc = lib.ampli_host_bam_scan(str(path).encode(), 2, stats)
        assert rc == 0, (case.name, lib.ampli_host_last_error())
        assert (stats[0], stats[3]) == (case.n_reads, 0), case.name


def test_every_wrong_variant_is_caught_by_a_deterministic_case():
    """Every variant of WRONG_VARIANTS must change the counts or the stats of at least one deterministic case (the fuzz streams do
    not count).  The list of catches is printed: run with -s to read it."""
    det = pm.deterministic_cases()
    right = [c.want() for c in det]
    uncaught = []
    for name, what in pm.WRONG_VARIANTS.items():
        caught = []
        for c, (counts, kept, added) in zip(det, right):
            w = c.want(wrong=name)
            if not np.array_equal(w[0], counts) or (w[1], w[2]) != (kept, added):
                caught.append(c.name)
        print(f"{name} ({what}): caught by {len(caught)} cases, first {caught[:3]}")
        if not caught:
            uncaught.append(name)
    assert not uncaught, f"no deterministic case notices: {uncaught}"


@pytest.mark.parametrize("variant,case", [
    ("window_last_key_dropped", "run_ends_on_the_last_window_key"), ("behind_window_dropped", "run_ends_one_past_the_window"),
    ("straddling_runs_dropped", "run_ends_one_past_the_window"), ("before_window_dropped", "second_read_starts_one_before_the_window"),
    ("unstaged_groups_dropped", "stage_over_phase0"), ("unstaged_groups_dropped", "only_middle_group_unstaged"),
    ("last_partial_group_dropped", "group_size_257"), ("last_read_dropped", "group_size_256"), ("mask_with_0x800", "each_flag_bit_alone"),
    ("reverse_from_0x20", "each_flag_bit_alone"), ("mbq_strict", "quality_around_mbq_255"), ("mrq_strict", "mapq_around_mrq_0"),
    ("nibble_parity_swapped", "match_runs_at_odd_and_even_query_offsets"), ("P_consumes_query", "all_nine_operations"),
    ("I_consumes_reference", "two_thousand_alternating_1M1I"), ("N_consumes_nothing", "deletions_and_skips_over_holes_and_keys")])
def test_the_edge_cases_catch_the_variant_they_were_built_for(variant, case):
    c = {c.name: c for c in pm.deterministic_cases()}[case]
    right, wrong = c.want(), c.want(wrong=variant)
    assert not np.array_equal(right[0], wrong[0]) or right[1:] != wrong[1:]


def test_the_edge_variants_leave_the_cases_off_the_edge_alone():
    """the window and stage variants are wrong ONLY on their edge: a case one step away from it must not notice"""
    det = {c.name: c for c in pm.deterministic_cases()}
    for variant, case in (("behind_window_dropped", "run_ends_on_the_last_window_key"), ("straddling_runs_dropped", "run_ends_on_the_last_window_key"),
                          ("unstaged_groups_dropped", "stage_exact_phase15"), ("unstaged_groups_dropped", "stage_under_phase0"),
                          ("window_last_key_dropped", "panel_of_%d_positions" % (pm.geometry().window - 1))):
        c = det[case]
        right, wrong = c.want(), c.want(wrong=variant)
        assert np.array_equal(right[0], wrong[0]) and right[1:] == wrong[1:], (variant, case)
