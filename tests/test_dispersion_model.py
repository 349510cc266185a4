"""The definition of the panel's dispersion (tests/dispersion_model.py) on its own: Haldane's moments by simulation, its K, D and n
against the CPU oracle's C = 0 table, and a planted contaminated normal."""
import numpy as np
import pytest

from oracle import pyoracle as orc
from tests.dispersion_cohorts import cohort, planted
from tests.dispersion_model import FEW, HIGH, cell_exact, dispersion_model, haldane_variance

ABSENT = np.iinfo(np.int32).min


@pytest.mark.parametrize("n,K", [(7, 3), (7, 40), (64, 5), (64, 500)])
def test_haldane_moments_by_simulation(n, K):
    """given K the counts are multinomial with probabilities d_i / D: X2 has mean n - 1 and variance V, at expected counts far below 1 too"""
    from fractions import Fraction

    rng = np.random.default_rng(20260 + n * 1000 + K)
    d = rng.integers(200, 5000, n)
    D = int(d.sum())
    k = rng.multinomial(K, d / D, size=200_000)
    e = K * d / D
    x2 = ((k - e) ** 2 / e).sum(axis=1)
    V = float(haldane_variance(n, K, D, sum(Fraction(1, int(v)) for v in d)))
    print(f"n={n} K={K}: mean {x2.mean():.4f} (n - 1 = {n - 1}), variance {x2.var():.2f} against V = {V:.2f} ({x2.var() / V - 1:+.2%})")
    assert V >= n - 1
    assert abs(x2.mean() - (n - 1)) <= 0.05
    assert abs(x2.var() / V - 1) <= 0.05


def test_one_pass_and_two_division_forms_agree_exactly():
    """(D / K) sum k^2 / d - K, which cell_exact evaluates, is sum (k - r d)^2 / (r d)"""
    from fractions import Fraction

    rng = np.random.default_rng(4)
    for _ in range(50):
        n = int(rng.integers(2, 12))
        k = [int(v) for v in rng.integers(0, 9, n)]
        d = [int(v) for v in rng.integers(100, 3000, n)]
        nn, K, D, x2, rinv, V = cell_exact(k, d)
        if K < 2:
            assert x2 is None
            continue
        r = Fraction(K, D)
        assert x2 == sum((ki - r * di) ** 2 / (r * di) for ki, di in zip(k, d))
        assert rinv == sum(Fraction(1, di) for di in d)


@pytest.mark.parametrize("P,S,extras,own_rd,cov", [(300, 7, False, False, 100), (130, 5, True, True, 30), (90, 2, True, False, 1)])
def test_totals_are_the_oracles_c0_table(P, S, extras, own_rd, cov):
    """snt, srd and cnt of the oracle's error_reduce with C = 0 are the model's K, D and n as integers: extras and own-RD lines included"""
    recs, E, dup_off, ext_pos, rd = cohort(P, S, 3 * P + S, extras=extras, own_rd=own_rd)
    acc = orc.error_reduce(recs, P, 0.0, cov, E=E, dup_off=dup_off, rd=rd)
    m = dispersion_model(recs, P, cov, E=E, ext_pos=ext_pos)
    assert acc["snt"].dtype == np.float64 and np.array_equal(acc["snt"], np.floor(acc["snt"]))
    assert np.array_equal(acc["snt"].astype(np.int64), m["K"])
    assert np.array_equal(acc["srd"], m["D"])
    assert np.array_equal(acc["cnt"].astype(np.int64), m["n"])
    assert (m["status"] != FEW).sum() > 0 or S < 3


def test_planted_normal_is_found():
    recs, spots = planted()
    S, P = recs.shape[0], recs.shape[1]
    bad = 4
    m = dispersion_model(recs, P, 100, z_cutoff=4.0)
    assert len(spots) == 20
    for p, nt in spots:
        assert m["status"][0, nt, p] & HIGH and m["status"][1, nt, p] & HIGH, (p, nt, m["z"][:, nt, p])
    ratio = m["sample_x2"] / m["sample_expect"]
    print("ratios:", np.round(ratio, 3))
    assert int(np.argmax(ratio)) == bad
    others = np.delete(ratio, bad)
    assert others.max() <= 0.5 * ratio[bad]
