"""The definition (tests/concordance_model.py) on a planted cohort: 12 samples drawn from 5 synthetic individuals at P = 600, about
15 % het sites per individual, binomial read noise at depth 300-3000; one individual is in both the normal and the tumour set.  Every
pair of samples of one individual must come out SAME, every other pair DIFFERENT -- and the model's pair counts, which come from
matrix products, must equal a loop over the positions."""
import numpy as np

from tests.concordance_cohorts import PLANTED_NORMALS, PLANTED_TUMOURS, planted, planted_counts
from tests.concordance_model import DIFFERENT, H, SAME, V, classify, format_files, pack_planes, pair_counts, planes, relations

MIN_SITES, SAME_FRACTION = 20, 0.8


def test_planted_cohort_same_and_different():
    recs, who = planted()
    assert recs.shape == (12, 600, 8) and len(set(who)) == 5 and set(PLANTED_NORMALS) & set(PLANTED_TUMOURS) == {0}
    bits = classify(recs)
    het_share = ((bits & H) != 0).mean(axis=1)
    assert (bits & V).all() and (0.10 < het_share).all() and (het_share < 0.20).all()
    counts = planted_counts()
    same = who[:, None] == who[None, :]
    # the precondition, on the model alone: every same-individual pair has enough het sites to be decided
    assert (counts[same][:, 3] >= MIN_SITES).all()
    rel = relations(counts, MIN_SITES, SAME_FRACTION)
    assert (rel[same] == SAME).all()
    assert (rel[~same] == DIFFERENT).all()


def test_pair_counts_equal_a_loop_over_positions():
    rng = np.random.default_rng(2)
    from tests.concordance_cohorts import records

    recs = records(77, 5, 9)
    bits = classify(recs)
    got = pair_counts(bits[:3], bits)
    for a in range(3):
        for b in range(5):
            c = [0] * 5
            for p in range(77):
                x, y = int(bits[a, p]), int(bits[b, p])
                if not (x & V and y & V):
                    continue
                sx, sy = (x >> 1) & 15, (y >> 1) & 15
                c[0] += 1
                c[1] += sx == sy
                c[2] += (sx & sy) == 0
                c[3] += bool((x | y) & H)
                c[4] += sx == sy and bool(x & H)
            assert got[a, b].tolist() == c
    assert rng is not None


def test_planes_layout_and_symmetry():
    from tests.concordance_cohorts import records

    P = 130
    recs = records(P, 4, 11)
    bits = classify(recs)
    pl = planes(recs, P)
    assert pl.shape == (4, 6, 3) and pl.dtype == np.uint64
    for s, k, p in ((0, 0, 0), (1, 1, 63), (2, 2, 64), (3, 5, 129), (0, 3, 128)):
        assert (int(pl[s, k, p // 64]) >> (p % 64)) & 1 == (int(bits[s, p]) >> k) & 1
    assert (pl[:, :, 2] >> np.uint64(2) == 0).all()  # bits at and beyond P
    assert ((pl[:, 1:] & ~pl[:, :1]) == 0).all()      # every plane is 0 where V is 0
    assert np.array_equal(pl, pack_planes(bits, P))
    c = pair_counts(bits, bits)
    assert np.array_equal(c, c.transpose(1, 0, 2))
    assert np.array_equal(np.diagonal(c[:, :, 0]), ((bits & V) != 0).sum(1)) and np.array_equal(np.diagonal(c[:, :, 3]), ((bits & H) != 0).sum(1))


def test_files_of_the_planted_cohort():
    recs, who = planted()
    names = [f"N{i}" for i in range(7)] + [f"T{i}" for i in range(5)]
    samples, pairs, summary = format_files(names, 7, planted_counts(), MIN_SITES, SAME_FRACTION)
    rows = [l.split("\t") for l in samples.splitlines()[1:]]
    assert [r[0] for r in rows] == names and [r[1] for r in rows] == ["N"] * 7 + ["T"] * 5
    for i, r in enumerate(rows):
        assert int(r[4]) == (who == who[i]).sum() - 1 and who[names.index(r[5])] == who[i] and float(r[8]) >= SAME_FRACTION
    n_same = int(sum((who == w).sum() * ((who == w).sum() - 1) // 2 for w in set(who)))
    assert len(pairs.splitlines()) == 1 + n_same and all(l.endswith("\tSAME") for l in pairs.splitlines()[1:])
    assert f"pairs_same={n_same}\npairs_different={66 - n_same}\npairs_undetermined=0\n" in summary and summary.startswith("normals=7\ntumours=5\nmin_depth=100\n")
