"""The read-evidence model against itself, on the CPU: the two restatements of the counting agree on every case, every deliberately wrong
variant is caught by its named deterministic cases, the invariant against the pileup model holds (per position, nt and metric the bins sum
to the pileup count), and the numpy score agrees with the exact one.  Needs the kernel's source text (its geometry), not the build."""
import numpy as np
import pytest

from tests import evidence_model as em
from tests import pileup_model as pm

CASES = em.cases()
BY_NAME = {c.name: c for c in CASES}
SCORE_BY_NAME = {c[0]: c for c in em.score_cases()}


def test_the_contracts_numbers_are_the_headers():
    geo = em.geometry()
    assert (geo.metrics, geo.bins, geo.bq, geo.mq, geo.pos) == (em.METRICS, em.BINS, em.BQ, em.MQ, em.POS) == (3, 64, 0, 1, 2)
    assert geo.reads == 256 and 1 <= geo.window <= 16


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_the_two_restatements_agree(case):
    got, want = em.walk(case.stream, case.keys, case.mbq, case.mrq), case.want()
    assert not em.differences(got, want)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_the_bins_of_every_metric_sum_to_the_pileup_count(case):
    counts, kept, added = pm.count(case.stream, case.keys, case.mbq, case.mrq)
    w = case.want()
    assert w.stats == (kept, added)
    for m in range(em.METRICS):
        assert np.array_equal(w.hist[:, :, m, :].sum(2), counts[:, :4])


@pytest.mark.parametrize("variant", sorted(em.COUNT_VARIANTS))
def test_every_wrong_count_is_caught_by_its_cases(variant):
    assert em.CAUGHT_BY[variant]
    for name in em.CAUGHT_BY[variant]:
        case = BY_NAME[name]
        assert em.differences(case.want(wrong=variant), case.want()), (variant, name)


@pytest.mark.parametrize("variant", sorted(em.SCORE_VARIANTS))
def test_every_wrong_score_is_caught_by_its_cases(variant):
    assert em.SCORE_CAUGHT_BY[variant]
    for name in em.SCORE_CAUGHT_BY[variant]:
        _, planes, ref, alt = SCORE_BY_NAME[name]
        assert em.score_differences(em.score(planes, ref, alt, wrong=variant), em.score(planes, ref, alt)), (variant, name)


def test_every_variant_has_cases():
    assert set(em.CAUGHT_BY) == set(em.COUNT_VARIANTS) and set(em.SCORE_CAUGHT_BY) == set(em.SCORE_VARIANTS)


def _against_exact(planes, ref, alt):
    """the numpy score of the planes against the exact one; returns (cells compared within 1e-10, cells near the cancellation)"""
    s = em.score(planes, ref, alt)
    far = near = 0
    for p in range(len(planes)):
        exact, used = em.score_exact(planes[p], int(ref[p]), int(alt[p]))
        assert used == s.alt_used[p]
        for m, e in enumerate(exact):
            assert s.ints[p, m, :2].tolist() == [e["n_ref"], e["n_alt"]] and s.med[p, m].tolist() == [e["med_ref"], e["med_alt"]]
            if e["c"] is not None and e["c"] >= em.Fraction(e["N"] + 1, 100):
                assert s.ints[p, m, 2] == e["u2"], (p, m, e)
                # at most about 200 roundings of 2^-53, amplified at most 100-fold by the one subtraction: 200 x 100 x 1.1e-16 < 1e-10
                z2 = em.Fraction(float(s.z2[p, m]))
                assert abs(z2 - e["z2"]) <= em.Fraction(1, 10 ** 10) * abs(e["z2"]), (p, m, float(z2), float(e["z2"]))
                far += 1
            else:  # nearer the cancellation: the untested rule where the exact factor decides it, and the sign
                if e["c"] is None or e["c"] == 0 or e["n_ref"] == 0 or e["n_alt"] == 0:
                    assert s.ints[p, m, 2] == -1 and s.z2[p, m] == 0.0
                if s.ints[p, m, 2] >= 0 and e["u2"] >= 0:
                    assert (s.z2[p, m] > 0) == (e["z2"] > 0) and (s.z2[p, m] < 0) == (e["z2"] < 0)
                near += 1
    return far, near


def test_the_score_cases_against_the_exact_score():
    for _, planes, ref, alt in em.score_cases():
        _against_exact(planes, ref, alt)


def test_random_planes_against_the_exact_score():
    planes, ref, alt = em.random_planes(np.random.default_rng(2901), 120)
    far, near = _against_exact(planes, ref, alt)
    assert far >= 100, (far, near)


def test_the_files_of_a_small_list():
    planes = np.stack([em.plane(A={40: 50, 41: 50}, C={20: 5, 21: 5}), em.plane(A={40: 50}, C={40: 3}), em.plane(G={30: 9})])
    ev, hist = em.files([("chr1", 100, "A", "C"), ("chr1", 200, "A", "."), ("chrUn", 5, "G", "AT")], planes, min_alt=4, z_min=3.0)
    lines = ev.splitlines()
    assert lines[0].split("\t")[:6] == ["chr1", "100", "A", "C", "100", "10"] and lines[0].endswith("\tLOW_BQ,LOW_MQ,READ_END")
    assert lines[1].split("\t") == ["chr1", "200", "A", "C", "50", "3", "40", "40", ".", "40", "40", ".", "40", "40", ".", "UNTESTED"]
    assert lines[2].split("\t") == ["chrUn", "5", "G", "AT", "9", "0", "30", "-1", ".", "30", "-1", ".", "30", "-1", ".", "UNTESTED"]
    assert hist.splitlines()[0] == "chr1\t100\tA\tBQ\t40\t50" and len(hist.splitlines()) == 3 * 4 + 3 * 2 + 3
