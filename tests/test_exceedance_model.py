"""The definition of the panel-of-normals exceedance (tests/exceedance_model.py) on hand-made records, one per clause; its additivity over
every split of the normals into chunks; and the planted cohort (tests/exceedance_cohorts.py) on it.

Measured on the planted cohort at the defaults (min_alt_reads 3, min_vaf_pm 0, min_normals 10, max_normals 0, cut-offs 100): all 40
planted variants of T_VAR are candidates for every min_alt_reads in 1..5; none of the 5 het-site variants of T_HET is, each with ge = 2
on both strands; T_SHALLOW and T_NONE are all NA.  The clean file has 3 candidates among 6138 evaluated cells (0.049 %) and the
leave-self-out run of the 24 normals 106 among 147 921 (0.072 %).  With min_alt_reads <= 1 the fractions are the resolution of the
statistic: 8 of 6138 = 0.13 % beside 1 / 25^2 = 0.16 %, and 266 of 147 921 = 0.18 % beside 1 / 24^2 = 0.17 %.  The bounds below are
twice the measured counts."""
import itertools

import numpy as np

from tests.exceedance_cohorts import CAND, N_NORMALS, T_CLEAN, T_HET, T_NONE, T_SHALLOW, T_VAR, planted, planted_results
from tests.exceedance_model import ABSENT, NA, candidates, evaluated, exceedance

GONE = [ABSENT, 0, 0, 0, 0, 0, 0, 0]


def rec(fw, bw):
    return list(fw) + list(bw)


def one(t, n, ref=0, **kw):
    """one tumour record against the normal records n at one position -> elig (a number), ge [4, 2]"""
    e, g = exceedance(np.array([[t]], np.int32), np.array([[x] for x in n], np.int32), np.array([ref], np.uint8), **kw)
    return int(e[0, 0]), g[0, 0].astype(int)


T = rec([900, 100, 0, 0], [450, 50, 0, 0])  # 10 % C on both strands, reference A


def test_absent_records():
    e, g = one(GONE, [T, T])
    assert e == 2 and (g == NA).all()                       # the tumour's record is absent: its normals are still counted
    e, g = one(T, [GONE, T, GONE])
    assert e == 1 and g[1].tolist() == [1, 1] and g[0].tolist() == [NA, NA]
    assert one(T, [GONE])[0] == 0 and one(T, [GONE])[1][1].tolist() == [0, 0]


def test_the_normal_cut_off_on_each_strand():
    for fw, bw, ok in ((99, 100, 0), (100, 99, 0), (100, 100, 1), (99, 99, 0), (101, 100, 1)):
        n = rec([fw - 50, 50, 0, 0], [bw - 50, 50, 0, 0])  # half C: reaches wherever it is eligible
        e, g = one(T, [n], normal_cutoff=100)
        assert e == ok and g[1].tolist() == [ok, ok], (fw, bw)
    assert one(T, [rec([1, 0, 0, 0], [0, 1, 0, 0])], normal_cutoff=1)[0] == 1


def test_the_calling_cut_off_on_each_strand():
    n = rec([500, 500, 0, 0], [500, 500, 0, 0])
    for fw, bw, ok in ((99, 100, False), (100, 99, False), (100, 100, True), (99, 99, False)):
        t = rec([fw - 10, 10, 0, 0], [bw - 10, 10, 0, 0])
        e, g = one(t, [n], calling_cutoff=100)
        assert e == 1 and (g[1:] != NA).all() == ok and (g[1:] == NA).all() == (not ok), (fw, bw)
        assert (g[0] == NA).all()


def test_the_reference_code():
    n = rec([500, 500, 0, 0], [500, 500, 0, 0])
    for ref in (255, 4, 17):
        e, g = one(T, [n], ref=ref)
        assert e == 1 and (g == NA).all()
    for ref in range(4):                                    # b == ref is NA on both strands, the other three bases are counted
        e, g = one(T, [n], ref=ref)
        assert (g[ref] == NA).all() and (np.delete(g, ref, 0) != NA).all()
    assert one(T, [n], ref=2)[1].tolist() == [[0, 0], [1, 1], [NA, NA], [1, 1]]  # A: 50 % < 90 %; C: 50 % >= 10 %; T: 0 >= 0


def test_equality_and_one_read_either_side():
    t = rec([970, 30, 0, 0], [485, 15, 0, 0])               # 3 % on both strands
    for k, reach in ((59, 0), (60, 1), (61, 1)):            # a normal of depth 2000: 60 reads are 3 %
        n = rec([2000 - k, k, 0, 0], [2000 - k, k, 0, 0])
        assert one(t, [n])[1][1].tolist() == [reach, reach], k
    n = rec([1940, 60, 0, 0], [1941, 59, 0, 0])             # the strands are separate
    assert one(t, [n])[1][1].tolist() == [1, 0]
    for k, reach in ((29, 1), (30, 1), (31, 0)):            # the tumour's read either side
        assert one(rec([1000 - k, k, 0, 0], [485, 15, 0, 0]), [rec([1940, 60, 0, 0], [1940, 60, 0, 0])])[1][1].tolist() == [reach, 1], k


def test_no_reads_in_the_tumour_and_no_depth_in_the_normal():
    n = [rec([500, 0, 0, 0], [500, 0, 0, 0]), rec([100, 1, 0, 0], [100, 0, 0, 0]), GONE]
    e, g = one(rec([200, 0, 0, 0], [200, 0, 0, 0]), n)
    assert e == 2 and g[1:].tolist() == [[2, 2]] * 3        # x_t == 0: every eligible normal reaches
    e, g = one(T, [[0] * 8], normal_cutoff=0)
    assert e == 1 and g[1:].tolist() == [[1, 1]] * 3        # D_s == 0 with a cut-off of zero: 0 >= 0
    e, g = one(T, [[0] * 8], normal_cutoff=1)
    assert e == 0 and g[1:].tolist() == [[0, 0]] * 3        # ... and stopped by a positive one
    e, g = one([0] * 8, [T], calling_cutoff=0, normal_cutoff=0)
    assert e == 1 and g[1:].tolist() == [[1, 1]] * 3        # D_t == 0 as well


def test_fields_of_two_to_the_thirty_one_minus_one():
    top = (1 << 31) - 1
    t = rec([top, top, top, top - 1], [top, top, top, top])
    same, less = rec([top, top, top, top - 1], [top, top, top, top]), rec([top, top - 1, top, top - 1], [top, top, top - 1, top])
    e, g = one(t, [same, less])
    assert e == 2
    # D_t[0] = 4 top - 1 > 2^32; x_s D_t and x_t D_s are near 2^64 / 2: a signed or a 32-bit product gets them wrong
    assert g[1].tolist() == [1, 2] and g[2].tolist() == [2, 1] and g[3].tolist() == [2, 2]
    assert int(top) * (4 * top - 1) < 1 << 64 and int(top) * (4 * top - 1) > 1 << 63
    small = rec([3, 1, 0, 0], [3, 1, 0, 0])                # 25 %: top / (4 top - 1) is a little more
    assert one(t, [small], normal_cutoff=0)[1][1].tolist() == [0, 1] and one(small, [t], calling_cutoff=0)[1][1].tolist() == [1, 1]


def test_skip_same_index():
    n = [rec([500, 500, 0, 0], [500, 500, 0, 0])] * 5
    t = np.array([[T]] * 3, np.int32)
    nn, ref = np.array([[x] for x in n], np.int32), np.array([0], np.uint8)
    for first_t, first_n, skipped in ((0, 0, [1, 1, 1]), (7, 5, [1, 1, 1]), (3, 5, [0, 0, 1]), (9, 5, [1, 0, 0]), (10, 5, [0, 0, 0]), (0, 3, [0, 0, 0])):
        e, g = exceedance(t, nn, ref, first_t=first_t, first_n=first_n, skip_same_index=True)
        assert e[:, 0].tolist() == [5 - k for k in skipped] and g[:, 0, 1, 0].tolist() == [5 - k for k in skipped], (first_t, first_n)
        e, g = exceedance(t, nn, ref, first_t=first_t, first_n=first_n, skip_same_index=False)
        assert e[:, 0].tolist() == [5, 5, 5] and g[:, 0, 1, 1].tolist() == [5, 5, 5]


def _random(P, n_t, n_n, seed):
    rng = np.random.default_rng(seed)
    ref = rng.choice([0, 1, 2, 3, 255], P).astype(np.uint8)
    recs = rng.choice([0, 1, 2, 3, 50, 100, 400], (n_t + n_n, P, 8)).astype(np.int32)
    recs[rng.random((n_t + n_n, P)) < 0.1] = GONE
    return recs[:n_t], recs[n_t:], ref


def test_additivity_over_every_split_of_the_normals():
    t, n, ref = _random(40, 3, 6, 1)
    for skip in (False, True):
        e1, g1 = exceedance(t, n, ref, first_t=2, first_n=1, skip_same_index=skip)
        assert (g1 == NA).any() and ((g1 != NA) & (g1 > 0)).any() and (e1 < 6).any()
        for k in range(6):
            for cuts in itertools.combinations(range(1, 6), k):
                edges = (0,) + cuts + (6,)
                e, g = None, None
                for lo, hi in zip(edges[:-1], edges[1:]):
                    e, g = exceedance(t, n[lo:hi], ref, first_t=2, first_n=1 + lo, skip_same_index=skip, elig=e, ge=g)
                assert np.array_equal(e, e1) and np.array_equal(g, g1), edges


def test_every_planted_variant_is_a_candidate():
    c, r = planted(), planted_results()
    row = T_VAR - N_NORMALS
    assert len(c["variants"]) == 40
    for mar in range(1, 6):
        cand = candidates(c["recs"][N_NORMALS:], r["elig"], r["ge"], **dict(CAND, min_alt_reads=mar))
        assert all(cand[row, p, y] for p, y in c["variants"]), mar  # all 40
    assert all((r["ge"][row, p, y] == 0).all() and r["elig"][row, p] >= 20 for p, y in c["variants"])


def test_no_het_site_variant_is_a_candidate():
    c, r = planted(), planted_results()
    row = T_HET - N_NORMALS
    assert len(c["hets"]) == 5
    for p, y in c["hets"]:
        assert not r["cand"][row, p, y] and (r["ge"][row, p, y] >= 2).any() and r["ge"][row, p, y].max() != NA
        assert not candidates(c["recs"][N_NORMALS:], r["elig"], r["ge"], **dict(CAND, min_alt_reads=1, max_normals=1))[row, p, y]


def test_shallow_and_empty_files_are_all_na():
    c, r = planted(), planted_results()
    for row in (T_SHALLOW - N_NORMALS, T_NONE - N_NORMALS):
        assert (r["ge"][row] == NA).all() and not r["cand"][row].any() and (r["elig"][row] >= 20).all()
    assert not evaluated(c["recs"][[T_SHALLOW, T_NONE]], c["ref_code"]).any()


def test_the_clean_fractions_stay_within_twice_the_measured_ones():
    c, r = planted(), planted_results()
    ev = evaluated(c["recs"][N_NORMALS:], c["ref_code"])
    row = T_CLEAN - N_NORMALS
    clean, cells = int(r["cand"][row].sum()), int(ev[row].sum())
    self_cand, self_cells = int(r["self_cand"].sum()), int(evaluated(c["recs"][:N_NORMALS], c["ref_code"]).sum())
    print(f"clean file: {clean} candidates of {cells} evaluated cells; leave-self-out: {self_cand} of {self_cells}")
    assert cells == 6138 and self_cells == 147921
    assert clean <= 2 * 3 and self_cand <= 2 * 106          # measured: 3 and 106
    assert (r["self_elig"] <= N_NORMALS - 1).all() and r["self_elig"].max() == N_NORMALS - 1 and r["elig"].max() == N_NORMALS
    # the resolution: without a floor on the reads, topping N normals on two strands has a chance of about 1 / (N + 1)^2
    loose = candidates(c["recs"][:N_NORMALS], r["self_elig"], r["self_ge"], **dict(CAND, min_alt_reads=0))
    assert 0.5 / 24 ** 2 < loose.sum() / self_cells < 2.0 / 24 ** 2
