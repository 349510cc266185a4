"""The definition of the contamination check (tests/contamination_model.py) on hand-made positions, one per row of the table of
include/amplisolve_hip.h, the estimate on its branches, and the planted cohort (tests/contamination_cohorts.py).

The planted bounds -- |fraction - c| <= 0.1 c + 0.0005 for a mixture's true source, below 0.0005 for every clean recipient -- come from
a trial of the definition on such a cohort.  Re-measured on the committed generator's draws: the worst relative error is 2.5 % (0.1525
for c = 0.15; 0.00011 absolute at c = 0.002, bound 0.0007) and the worst clean value 0.00017: both bounds keep more than a 2 x margin
over the observed worst case."""
import math

import numpy as np

from tests.concordance_model import ABSENT, A, C, G, H, T, V, classify
from tests.contamination_cohorts import MIXTURES, N_INDIVIDUALS, planted, planted_sums
from tests.contamination_model import (ALT_BG, ALT_HET, ALT_HOM, CLEAN, CONTAMINATED, DEPTH_BG, DEPTH_HET, DEPTH_HOM, SITES_BG, SITES_HET,
                                       SITES_HOM, UNDETERMINED, estimate, format_files, status, statuses, sums)

REC = [400, 3, 5, 7, 500, 11, 13, 17]  # n = A 900, C 14, G 18, T 24; d = 956
N_, D_ = [900, 14, 18, 24], 956


def _one(bit_a, bit_b, rec=REC):
    return sums(np.array([[rec]], np.int32), np.array([[bit_a]], np.uint8), np.array([[bit_b]], np.uint8))[0, 0].tolist()


def test_the_record_classifies_as_the_recipient_of_every_row():
    assert classify(np.array([REC], np.int32))[0] == V | A


def test_one_position_per_row_of_the_table():
    assert _one(V | A, V | C) == [1, N_[1], D_, 0, 0, 0, 0, 0, 0]                       # b homozygous for another base
    assert _one(V | A, V | T) == [1, N_[3], D_, 0, 0, 0, 0, 0, 0]
    assert _one(V | A, V | H | A | G) == [0, 0, 0, 1, N_[2], D_, 0, 0, 0]               # b het with one non-X base
    assert _one(V | A, V | H | C | T) == [0, 0, 0, 1, N_[1] + N_[3], 2 * D_, 0, 0, 0]   # b het with two non-X bases: two slots
    assert _one(V | A, V | A) == [0, 0, 0, 0, 0, 0, 1, D_ - N_[0], D_]                  # b has a's genotype: the background
    assert _one(V | C, V | C) == [0, 0, 0, 0, 0, 0, 1, D_ - N_[1], D_]


def test_a_het_or_invalid_adds_nothing():
    for bit_a in (V | H | A | C, 0, H | A | C, A):
        for bit_b in (V | C, V | H | A | G, V | A, 0):
            assert _one(bit_a, bit_b) == [0] * 9, (bit_a, bit_b)


def test_b_invalid_adds_nothing():
    for bit_b in (0, C, H | C | G):
        assert _one(V | A, bit_b) == [0] * 9


def test_an_absent_record_under_a_set_v_bit_counts_sites_and_zeros():
    gone = [ABSENT, 3, 5, 7, 500, 11, 13, 17]
    assert _one(V | A, V | C, gone) == [1, 0, 0, 0, 0, 0, 0, 0, 0]
    assert _one(V | A, V | H | C | T, gone) == [0, 0, 0, 1, 0, 0, 0, 0, 0]
    assert _one(V | A, V | A, gone) == [0, 0, 0, 0, 0, 0, 1, 0, 0]


def test_a_sample_against_itself_has_background_only():
    recs, _ = planted()
    bits = classify(recs)
    S = planted_sums()
    hom = ((bits & V) != 0) & ((bits & H) == 0)
    for i in range(len(recs)):
        assert (S[i, i, :SITES_BG] == 0).all() and S[i, i, SITES_BG] == hom[i].sum() > 300
        d = recs[i].astype(np.int64).sum(-1)
        assert S[i, i, DEPTH_BG] == d[hom[i]].sum() and 0 < S[i, i, ALT_BG] < S[i, i, DEPTH_BG] // 50
        assert status(S[i, i], 1, 0.005) == UNDETERMINED and math.isnan(estimate(S[i, i])[0])


def test_sums_add_over_positions_and_pairs_are_independent():
    recs, _ = planted()
    bits = classify(recs)
    S = planted_sums()
    a, b = sums(recs[2:5, :100], bits[2:5, :100], bits[7:, :100]), sums(recs[2:5, 100:], bits[2:5, 100:], bits[7:, 100:])
    assert np.array_equal(a + b, S[2:5, 7:])


def test_estimate_branches():
    s = [0] * 9
    f, se, e = estimate(s)
    assert math.isnan(f) and math.isnan(se) and e == 0.0                                # den == 0
    s = [10, 50, 5000, 0, 0, 0, 0, 0, 0]
    assert estimate(s) == (0.01, math.sqrt(50.0) / 5000.0, 0.0)                         # s8 == 0: no background
    s = [10, 50, 5000, 4, 30, 4000, 100, 300, 100000]
    e = 300.0 / (3.0 * 100000.0)
    assert estimate(s) == ((80.0 - e * 9000.0) / 7000.0, math.sqrt(80.0) / 7000.0, e)   # het depth counts half in den, whole in slots
    s = [10, 2, 5000, 0, 0, 0, 100, 900, 100000]
    f, se, e = estimate(s)
    assert f == 0.0 and math.copysign(1.0, f) == 1.0 and se == math.sqrt(2.0) / 5000.0  # num < 0 clamps to +0
    assert estimate([0, 0, 0, 5, 7, 0, 0, 0, 0])[0] != estimate([0, 0, 0, 5, 7, 0, 0, 0, 0])[0]  # het sites without depth: NaN


def test_status():
    s = [12, 50, 5000, 8, 0, 0, 0, 0, 0]
    assert status(s, 21, 0.005) == UNDETERMINED and status(s, 20, 0.005) == CONTAMINATED and status(s, 20, 0.01) == CONTAMINATED
    assert status(s, 20, 0.0101) == CLEAN
    assert status([30, 0, 0, 0, 0, 0, 0, 0, 0], 20, 0.005) == CLEAN  # sites without depth: a NaN is never >= min_fraction


def test_planted_cohort():
    S = planted_sums()
    _, who = planted()
    N = len(who)
    F = np.array([[estimate(S[i, j])[0] for j in range(N)] for i in range(N)])
    st = statuses(S, 20, 0.005)
    for k, (r, s, c) in enumerate(MIXTURES):
        i = N_INDIVIDUALS + k
        if r == s:
            continue
        ranked = np.where(st[i] != UNDETERMINED, F[i], -1.0)
        assert who[int(np.argmax(ranked))] == s, (r, s, c, F[i])
        print(f"mixture {r} <- {s} at {c}: fraction {F[i, s]:.5f}, off by {abs(F[i, s] - c):.5f} of {0.1 * c + 0.0005:.5f}")
        assert abs(F[i, s] - c) <= 0.1 * c + 0.0005
        assert st[i, s] == (CONTAMINATED if c >= 0.005 else CLEAN)
    clean = list(range(N_INDIVIDUALS)) + [N_INDIVIDUALS + k for k, (r, s, c) in enumerate(MIXTURES) if r == s]
    assert len(clean) == 7
    worst = max(F[i, j] for i in clean for j in range(N) if F[i, j] == F[i, j])
    print(f"worst clean fraction {worst:.5f}")
    for i in clean:
        for j in range(N):
            assert not F[i, j] >= 0.0005, (i, j, F[i, j])
            assert st[i, j] == (UNDETERMINED if who[i] == who[j] else CLEAN)              # one individual: no informative site


def test_format_files_on_the_planted_cohort():
    S = planted_sums()
    names = [f"S{i:02d}" for i in range(12)]
    samples, pairs, summary = format_files(names, 7, S, 20, 0.005)
    rows = samples.splitlines()
    assert rows[0].split("\t") == ["Sample", "Set", "HomSites", "Background", "Source", "Sites", "Fraction", "SE", "Status"] and len(rows) == 13
    assert rows[1].split("\t")[:2] == ["S00", "N"] and rows[8].split("\t")[:2] == ["S07", "T"]
    assert rows[7].split("\t")[4] == "S01" and rows[7].endswith("\tCONTAMINATED") and rows[1].endswith("\tCLEAN")  # S06 = 0 + 1 % of 1
    assert rows[12].split("\t")[4] == "S02" and rows[12].split("\t")[6].startswith("0.15")
    st = statuses(S, 20, 0.005)
    off = ~np.eye(12, dtype=bool)
    assert len(pairs.splitlines()) == 1 + int((st[off] == CONTAMINATED).sum()) and "S06\tS01\t51\t857\t" in pairs
    assert summary.startswith("normals=7\ntumours=5\nmin_depth=100\n") and "min_sites=20\nmin_fraction=0.005\n" in summary
    assert summary.endswith(f"pairs_contaminated={(st[off] == CONTAMINATED).sum()}\npairs_clean={(st[off] == CLEAN).sum()}\n"
                            f"pairs_undetermined={(st[off] == UNDETERMINED).sum()}\n")
    # nobody determined: NA
    lone = format_files(["X"], 1, S[:1, :1], 20, 0.005)
    assert lone[0].splitlines()[1].endswith("\tNA\tNA\tNA\tNA\tUNDETERMINED") and lone[1].count("\n") == 1
