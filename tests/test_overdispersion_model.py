"""The definition of overdispersion-aware calling (tests/overdispersion_model.py) checked against itself: the moment
identity behind omega by simulation, hand-made cells for every clause of the fit, the tail against closed forms and against scipy, and
the host library's export of the cell arithmetic (ampli_host_overdispersion_cell_batch) on the same cells."""
import ctypes as C
from fractions import Fraction

import mpmath as mp
import numpy as np

from amplisolve_amd import host_lib
from tests.dispersion_model import FEW, HIGH, OK, cell_exact
from tests.overdispersion_model import nb_q, nb_tail, omega_bound, omega_exact


def _host_omega(status, n, K, D, x2, s2):
    a = [np.ascontiguousarray(status, np.uint8), np.ascontiguousarray(n, np.int32)] + [np.ascontiguousarray(v, np.float64) for v in (K, D, x2, s2)]
    out = np.full(len(a[0]), np.nan)
    host_lib().ampli_host_overdispersion_cell_batch(*[v.ctypes.data_as(C.c_void_p) for v in a], len(out), out.ctypes.data_as(C.c_void_p))
    return out


def _cell(k, d, status):
    n, K, D, x2, _, _ = cell_exact(k, d)
    return status, n, K, D, float(x2) if x2 is not None else 0.0, sum(v * v for v in d)


# one cell per clause: (counts, depths, status fed in, the clause)
CELLS = [
    ([5], [1000], FEW, "n < 2"),
    ([1, 0, 0], [900, 1000, 1100], FEW, "K < 2"),
    ([2, 3, 2, 3], [1000, 1100, 900, 1000], OK, "not HIGH"),
    ([0, 40, 1, 0], [1000, 1100, 900, 1000], HIGH, "HIGH"),
    ([30, 0, 1], [60000, 3, 2], HIGH, "a single dominating depth"),
    ([7], [1000], HIGH, "D - S2 / D == 0 (one record, whatever the status says)"),
    ([3, 0], [1, 1], HIGH, "D - S2 / D at its smallest for two records"),
]


def test_every_clause_of_the_fit():
    rows = [_cell(k, d, st) for k, d, st, _ in CELLS]
    got = _host_omega(*zip(*rows))
    for (status, n, K, D, x2, s2), g, (_, _, _, what) in zip(rows, got, CELLS):
        w = omega_exact(status, n, K, D, x2, s2)
        if not status & HIGH or D * D == s2:
            assert w == 0 and g == 0.0, what
        else:
            assert w > 0, what  # a HIGH cell of these has X2 > n - 1
            print(what, float(w), g, abs(g - float(w)), omega_bound(w, D, s2))
            assert abs(Fraction(g) - w) <= Fraction(omega_bound(w, D, s2)), what
    # the dominating depth: D - S2 / D is 10 of D = 60005, and the bound grows with S2 / (D^2 - S2)
    _, n, K, D, x2, s2 = rows[4]
    assert 0 < D - Fraction(s2, D) < 11 and s2 / (D * D - s2) > 1000


def test_a_quotient_that_is_not_above_zero_is_zero():
    # HIGH with X2 < n - 1: what a negative z_cutoff produces
    assert _host_omega([HIGH], [4], [10.0], [4000.0], [1.5], [4.0e6])[0] == 0.0
    assert omega_exact(HIGH, 4, 10, 4000, 1.5, 4000000) == 0


def test_moment_identity_by_simulation():
    """E[X2] = (n - 1) + omega r (D - S2 / D) under k_i ~ Poisson(lambda_i d_i), E lambda_i = r, Var lambda_i = omega r^2"""
    rng = np.random.default_rng(3)
    n, r, draws = 24, 0.004, 40000
    d = rng.integers(500, 4000, n).astype(np.float64)
    D, S2 = d.sum(), (d * d).sum()
    for omega in (0.5, 0.1):
        lam = r * rng.gamma(1 / omega, omega, size=(draws, n))
        k = rng.poisson(lam * d)
        K = k.sum(axis=1)
        ok = K >= 2
        x2 = (D / K[ok]) * (k[ok] ** 2 / d).sum(axis=1) - K[ok]
        want = (n - 1) + omega * r * (D - S2 / D)
        print(omega, x2.mean(), want)
        assert abs(x2.mean() - want) <= 0.04 * want  # the estimator conditions on K: a few per cent low


def test_tail_closed_forms():
    with mp.workdps(40):
        for m, w in ((0.3, 0.0), (7.0, 0.0), (0.3, 2.0), (7.0, 0.25), (1e4, 1e-8)):
            p0 = mp.exp(-mp.mpf(m)) if w == 0 else (1 + mp.mpf(m) * mp.mpf(w)) ** (-1 / mp.mpf(w))
            assert abs(nb_tail(1, m, w) - (1 - p0)) < mp.mpf(10) ** -35
            p1 = p0 * mp.mpf(m) / (1 + mp.mpf(m) * mp.mpf(w))
            assert abs(nb_tail(2, m, w) - (1 - p0 - p1)) < mp.mpf(10) ** -35
        # omega = 1 is the geometric law: P[X >= k] = (m / (1 + m))^k; the upward sum too (k far beyond what the complement is used for)
        for m, k in ((0.5, 3), (4.0, 10), (0.5, 400)):
            assert abs(nb_tail(k, m, 1.0) / (mp.mpf(m) / (1 + mp.mpf(m))) ** k - 1) < mp.mpf(10) ** -25
    assert nb_tail(0, 3.0, 0.5) == 1


def test_tail_against_scipy():
    from scipy import stats

    for m, w, k in ((2.0, 0.5, 6), (40.0, 1.5, 200), (3.0, 0.01, 9), (0.4, 10.0, 3), (1000.0, 0.02, 1500)):
        s = 1 / w
        ref = stats.nbinom.sf(k - 1, s, s / (s + m))
        assert abs(float(nb_tail(k, m, w)) / ref - 1) < 1e-9, (m, w, k)
    assert abs(float(nb_tail(9, 3.0, 0.0)) / stats.poisson.sf(8, 3.0) - 1) < 1e-12


def test_score_rules():
    assert nb_q(5, 1000, -1.0, 0.0) == np.float32(-888) and nb_q(0, 1000, -1.0, 0.0) == np.float32(-888)
    assert nb_q(0, 1000, 0.002, 1.5) == 0
    for bad in (-1e-9, float("nan"), float("inf")):
        assert nb_q(5, 1000, 0.002, bad) == np.float32(-1)
    assert nb_q(3, 1000, 0.0, 0.0) == nb_q(3, 1000, np.float32(0.0010008), 0.0)
    assert nb_q(60, 1000, 0.002, 0.0) == 100 and 0 < nb_q(3, 1000, 0.002, 0.0) < 100
    assert nb_q(9, 1000, 0.002, 1.5) < nb_q(9, 1000, 0.002, 0.0)  # the heavier tail scores lower
