"""The definition of the amplicon coverage check (tests/amplicon_model.py) on hand-made lists, one test per clause, and on the planted
cohort (tests/amplicon_cohorts.py).  The bounds of the planted cohort were measured on this model before they were written:
worst |ratio - planted| over the autosomal OK amplicons of all 17 files 0.0747 (bound 0.15), worst |z| over the clean cells 16.06
(bound 33)."""
import math

import numpy as np

from tests.amplicon_cohorts import (A, DROPPED_AMPLICON, GAIN_GENE, GENES, LOSS_GENE, N_NORMALS, T_BIG, T_DROP, T_GAIN, T_LOSS, T_MALE, ZERO_AMPLICON,
                                    lists_from_cover, planted, planted_results)
from tests.amplicon_model import (ABSENT, CALLABLE, DARK, DEPTH_BW, DEPTH_FW, FEW, GAIN, LOSS, NEUTRAL, OK, PRESENT, depth_sums, gene_status, genes, median,
                                  median_nan, ratios, reference, same, totals, z_of)

RATIO_BOUND, Z_BOUND = 0.15, 33.0


def _recs(rows):
    return np.array(rows, np.int64).astype(np.int32)[None]


def test_depth_sums_clause_by_clause():
    r = _recs([[100, 0, 0, 0, 50, 50, 0, 0], [ABSENT, 9, 9, 9, 9, 9, 9, 9], [1, 2, 3, 4, 5, 6, 7, 8], [99, 0, 0, 0, 100, 0, 0, 0], [100, 0, 0, 0, 99, 0, 0, 0],
               [25, 25, 25, 25, 100, 0, 0, 0]])
    # one list per clause: a present record; an absent one; an entry listed twice; an empty list; two overlapping lists; the gate
    off, pos = [0, 1, 2, 4, 4, 6, 8, 9, 10, 11], [0, 1, 2, 2, 0, 2, 2, 5, 3, 4, 5]
    s = depth_sums(r, off, pos, 100)[0]
    assert s[0].tolist() == [1, 100, 100, 1]
    assert s[1].tolist() == [0, 0, 0, 0]                      # an absent record adds nothing
    assert s[2].tolist() == [2, 20, 52, 0]                    # listed twice: counted twice
    assert s[3].tolist() == [0, 0, 0, 0]                      # an empty list
    assert s[4].tolist() == [2, 110, 126, 1] and s[5].tolist() == [2, 110, 126, 1]  # overlapping lists each count the shared position
    assert s[6].tolist() == [1, 99, 100, 0] and s[7].tolist() == [1, 100, 99, 0]    # cut-off - 1 on either strand
    assert s[8].tolist() == [1, 100, 100, 1]                                        # at the cut-off on both
    assert depth_sums(r, off, pos, 101)[0, 8].tolist() == [1, 100, 100, 0] and depth_sums(r, off, pos, 0)[0, 1].tolist() == [0, 0, 0, 0]
    assert s.dtype == np.int64


def test_depth_sums_are_additive_over_a_split_of_a_list():
    c = planted()
    rng = np.random.default_rng(1)
    pos = rng.integers(0, c["P"], 700)
    whole = depth_sums(c["recs"], [0, 700], pos)
    cut = depth_sums(c["recs"], [0, 123, 123, 700], pos)
    assert np.array_equal(whole[:, 0], cut.sum(1)) and (cut[:, 1] == 0).all()
    assert np.array_equal(whole, depth_sums(c["recs"], [0, 700], rng.permutation(pos)))  # and do not depend on the order


def test_median():
    assert math.isnan(median([]))
    assert median([3.0]) == 3.0 and median([1.0, 2.0]) == 1.5 and median([9.0, 1.0, 5.0]) == 5.0 and median([4.0, 1.0, 3.0, 2.0]) == 2.5
    assert median([2.0, 2.0, 2.0, 7.0]) == 2.0 and median([0.0, 0.0, 1.0]) == 0.0 and median([1.0, 7.0, 7.0, 9.0]) == 7.0
    a, b = 0.1, 0.30000000000000004
    assert median([b, a]) == (a + b) * 0.5
    assert median_nan([np.nan, -3.0, 5.0, np.nan, -1.0]) == -1.0 and math.isnan(median_nan([np.nan]))


def _sums(d):
    """depth matrix [n, A] -> sums with everything on the forward strand"""
    d = np.asarray(d, np.int64)
    s = np.zeros(d.shape + (4,), np.int64)
    s[:, :, DEPTH_FW] = d
    return s


def test_reference_statuses_at_their_bounds():
    d = np.array([[10, 30, 0], [20, 20, 0], [10, 10, 0], [0, 0, 0], [30, 10, 0]])
    use = np.ones(3, np.uint8)
    ref = reference(_sums(d), use, 4)
    assert ref["total"].tolist() == [40, 40, 20, 0, 40] and ref["n_eff"] == 4          # the empty normal is not included
    assert ref["status"].tolist() == [OK, OK, DARK]                                     # N_eff == min_normals; med == 0
    assert ref["med"].tolist() == [0.5, 0.5, 0.0] and ref["mad"].tolist()[:2] == [0.125, 0.125] and ref["mad"][2] == 0.0
    assert reference(_sums(d), use, 5)["status"].tolist() == [FEW] * 3                  # N_eff == min_normals - 1: before DARK
    none = reference(_sums(d * 0), use, 1)
    assert none["n_eff"] == 0 and none["status"].tolist() == [FEW] * 3 and np.isnan(none["med"]).all() and np.isnan(none["mad"]).all()
    masked = reference(_sums(d), np.array([1, 0, 0], np.uint8), 1)
    assert masked["total"].tolist() == [10, 20, 10, 0, 30] and masked["med"].tolist() == [1.0, 1.0, 0.0]


def test_ratios_t_zero_k_zero_and_mad_zero():
    d = np.array([[10, 30, 0, 40], [20, 20, 0, 40], [10, 10, 0, 20], [30, 10, 0, 40]])
    use = np.array([1, 1, 1, 0], np.uint8)
    ref = reference(_sums(d), use, 2)
    assert ref["mad"][3] == 0.0 and ref["status"].tolist() == [OK, OK, DARK, OK]
    rat = ratios(_sums(np.vstack([d, [[0, 0, 0, 7]]])), use, ref)
    assert rat["k"].tolist() == [2, 2, 2, 2, 0] and rat["total"][4] == 0
    assert np.isnan(rat["ratio"][4]).all() and np.isnan(rat["z"][4]).all() and math.isnan(rat["centre"][4])   # T == 0
    assert np.isnan(rat["ratio"][:, 2]).all()                                                                    # a DARK amplicon
    assert np.isnan(rat["z"][:, 3]).all() and not np.isnan(rat["ratio"][:4, 3]).any()                           # mad == 0: z is NaN
    none = ratios(_sums(d), np.zeros(4, np.uint8), ref)
    assert none["k"].tolist() == [0] * 4 and np.isnan(none["ratio"]).all()                                       # T == 0 for everyone
    dark = dict(ref, status=np.array([DARK, FEW, DARK, OK], np.uint8))
    k0 = ratios(_sums(d), use, dark)
    assert k0["total"].tolist() == [40, 40, 20, 40] and k0["k"].tolist() == [0] * 4                              # K == 0 with T > 0
    assert np.isnan(k0["centre"]).all() and np.isnan(k0["ratio"]).all()
    assert z_of(1.5, 0.25, 0.0) != z_of(1.5, 0.25, 0.0) and z_of(1.5, 0.25, 0.125) == (0.5 * 0.25) / (1.4826 * 0.125)


def test_gene_status_at_its_bounds():
    kw = dict(min_amplicons=3, gain_ratio=1.3, loss_ratio=0.7, z_cutoff=3.0)
    assert gene_status(3, 1.3, 3.0, **kw) == GAIN and gene_status(2, 1.3, 3.0, **kw) == NEUTRAL
    assert gene_status(3, 1.2999, 9.0, **kw) == NEUTRAL and gene_status(3, 2.0, 2.999, **kw) == NEUTRAL
    assert gene_status(3, 0.7, -3.0, **kw) == LOSS and gene_status(3, 0.7001, -9.0, **kw) == NEUTRAL and gene_status(3, 0.5, -2.9, **kw) == NEUTRAL
    assert gene_status(5, float("nan"), 9.0, **kw) == NEUTRAL and gene_status(5, 2.0, float("nan"), **kw) == NEUTRAL


def test_lists_leave_out_the_positions_two_amplicons_share():
    off, pos = lists_from_cover([(0, 5), (3, 5), (8, 2), (8, 2)], 10)
    assert off.tolist() == [0, 3, 6, 8, 10] and pos.tolist() == [0, 1, 2, 5, 6, 7, 8, 9, 8, 9]  # nothing left of its own: all entries


def test_planted_cohort():
    c, r = planted(), planted_results()
    ref, rat, g = r["ref"], r["rat"], r["genes"]
    status = ref["status"]
    assert status[ZERO_AMPLICON] == DARK and (np.delete(status, ZERO_AMPLICON) == OK).all() and ref["n_eff"] == N_NORMALS
    for (s, gene), (n, mr, mz, st) in g.items():
        if s < N_NORMALS or gene.startswith("X"):
            continue
        want = GAIN if (s, gene) == (T_GAIN, GAIN_GENE) else LOSS if (s, gene) == (T_LOSS, LOSS_GENE) else NEUTRAL
        assert st == want, (s, gene, n, mr, mz)
    assert all(g[s, gene][3] == NEUTRAL for s in range(N_NORMALS) for gene in GENES if not gene.startswith("X"))
    assert g[T_MALE, "X0"][1] < 0.75 and g[T_BIG, "X0"][1] > 1.25  # against normals of both sexes
    drop = r["sums"][T_DROP, DROPPED_AMPLICON]
    assert drop[CALLABLE] < drop[PRESENT] and drop[CALLABLE] == 0 and g[T_DROP, c["gene_of"][DROPPED_AMPLICON]][3] == NEUTRAL
    auto = (c["use"] != 0) & (status == OK)
    err = np.abs(rat["ratio"] - c["planted"])[:, auto]
    print("worst |ratio - planted|", err.max())
    assert err.max() < RATIO_BOUND
    clean = np.broadcast_to(auto, rat["z"].shape).copy()
    clean[T_GAIN, [x == GAIN_GENE for x in c["gene_of"]]] = False
    clean[T_LOSS, [x == LOSS_GENE for x in c["gene_of"]]] = False
    clean[T_DROP, DROPPED_AMPLICON] = False
    print("worst clean |z|", np.abs(rat["z"][clean]).max())
    assert np.abs(rat["z"][clean]).max() < Z_BOUND


def test_ratios_do_not_depend_on_the_library_size():
    c, r = planted(), planted_results()
    sums = r["sums"][[T_BIG]]
    tripled = ratios(sums * 3, c["use"], r["ref"])
    once = ratios(sums, c["use"], r["ref"])
    assert same(tripled["ratio"], once["ratio"]) and same(tripled["z"], once["z"]) and tripled["centre"][0] == once["centre"][0]
    assert np.array_equal(totals(sums * 3, c["use"]), 3 * totals(sums, c["use"]))
    auto = (c["use"] != 0) & (r["ref"]["status"] == OK)
    assert np.abs(r["rat"]["ratio"][T_BIG, auto] - 1.0).max() < RATIO_BOUND  # the file drawn at three times the library size
    assert A == 40 and len(genes(r["rat"]["ratio"], r["rat"]["z"], r["ref"]["status"], c["gene_of"])) == 17 * 8
