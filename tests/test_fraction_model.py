"""The definition of the tumour fraction (tests/fraction_model.py) against an independent reference, without the libraries: the model's
F_HAT, F_LO and F_HI against the roots of U = 0 and T = +-z2 found in mpmath at 50 digits, on the recorded grid
(tests/golden/fraction/grid.npz, written by python -m tests.fraction_model: lists of 1 to 300 entries, depths 1e2 to 1e7, f from 1e-5 to
0.5); and the interval's coverage in simulation.

The contract.  A bisection of 60 steps on [0, 1] ends 2^-61 = 4.3e-19 from its root, which is 2e-13 of the smallest roots of the grid
(2e-6); the rounding of the sums adds to that.  The worst relative deviation measured on the grid is 1.64e-13 (F_HAT; F_LO 1.2e-14, F_HI
3.1e-14); the contract is the next power of ten above it, REL = 1e-12."""
import os

import numpy as np
import pytest

from tests import fraction_model as fm

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fraction", "grid.npz")
REL = 1e-12


@pytest.fixture(scope="module")
def grid():
    lists, roots = fm.read_golden(GOLDEN)
    est = np.zeros((len(lists), 4))
    by_m = {}
    for i, x in enumerate(lists):
        by_m.setdefault(len(x[3]), []).append(i)
    for idx in by_m.values():  # lists of one length run side by side
        est[idx] = fm.solve(fm.cells_from_counts(*(np.stack([lists[i][j] for i in idx]) for j in range(4))))
    return lists, roots, est


def test_the_grid_is_the_one_the_model_draws(grid):
    lists, roots, _ = grid
    drawn = fm.grid_lists()
    assert len(lists) == len(drawn) == len(fm.GRID_M) * len(fm.GRID_DEPTH) * len(fm.GRID_F) == 396
    for got, want in zip(lists[::37], drawn[::37]):
        assert all(np.array_equal(g, w) for g, w in zip(got, want))
    assert {len(x[3]) for x in lists} == set(fm.GRID_M) and max(int(x[1].max()) for x in lists) > 1e7 and min(int(x[1].min()) for x in lists) < 100
    for i in (0, 5, 40, 77, 150, 215):  # the recorded roots are the reference's: recomputed here
        want = [np.nan if x is None else x for x in fm.exact_roots(*lists[i])]
        assert np.array_equal(np.array(want), roots[i], equal_nan=True)


def test_the_estimate_and_its_interval_against_fifty_digits(grid):
    _, roots, est = grid
    have = ~np.isnan(roots)
    assert have[:, 0].sum() > 340 and have[:, 1].sum() > 280 and have[:, 2].sum() > 340  # most of the grid has all three roots
    worst = [np.abs(est[have[:, v], v] - roots[have[:, v], v]) / roots[have[:, v], v] for v in range(3)]
    print("worst relative deviation of F_HAT, F_LO, F_HI:", [float(w.max()) for w in worst])
    for v in range(3):
        assert worst[v].max() <= REL, (v, worst[v].max())
    # where a first rule decides instead of a root, the model gives the rule's value
    no_hat = ~have[:, 0]
    assert (np.isin(est[no_hat, fm.F_HAT], (0.0, 1.0))).all() and (est[~have[:, 1], fm.F_LO][est[~have[:, 1], fm.F_HAT] < 1] == 0).all()
    assert (est[:, fm.F_LO] <= est[:, fm.F_HAT]).all() and (est[:, fm.F_HAT] <= est[:, fm.F_HI]).all()


def test_sums_in_the_lane_order_not_in_any_other():
    """the butterfly and the lane order are what the model adds in: a list of 130 entries, against the same terms added in the list's
    order (which differs in the last bits) and against 50 digits (which both are close to)"""
    import mpmath as mp

    k, d, e, a = fm.grid_lists()[-1 - 6 * 6]  # a list of 130 entries
    assert len(a) == 130
    c = fm.cells_from_counts(k[None], d[None], e[None], a[None])
    f = 0.0123
    U, I = fm.sums_at(c, np.array([f]))
    u = i = np.float64(0)
    for j in range(130):
        for st in range(2):
            g = np.float64(a[j]) / (np.float64(e[j, st]) + np.float64(f) * np.float64(a[j]))
            u = u + (g * np.float64(k[j, st]) - np.float64(a[j]) * np.float64(d[j, st]))
            i = i + g * (np.float64(a[j]) * np.float64(d[j, st]))
    with mp.workdps(50):
        xu = sum(mp.mpf(float(a[j])) / (mp.mpf(float(e[j, st])) + mp.mpf(f) * mp.mpf(float(a[j]))) * int(k[j, st]) - mp.mpf(float(a[j])) * int(d[j, st])
                 for j in range(130) for st in range(2))
        scale = sum(mp.mpf(float(a[j])) * int(d[j, st]) for j in range(130) for st in range(2))
        assert abs(mp.mpf(float(U[0])) - xu) < 1e-13 * scale and abs(mp.mpf(float(u)) - xu) < 1e-13 * scale
    assert (U[0], I[0]) != (u, i)  # not the same bits: the order is part of the definition
    lanes = np.zeros(64)
    lanes[3], lanes[35], lanes[2] = 1.0, 2.0 ** -53, 2.0 ** -53
    # lane 3 meets lane 35 first (off = 32) and lane 2 last (off = 1): 1 + 2^-53 rounds to 1 both times; the two small ones first give 1 + 2^-52
    assert fm.butterfly(lanes[None])[0] == 1.0 and (lanes[35] + lanes[2]) + lanes[3] == 1.0 + 2.0 ** -52
    assert fm.butterfly(np.arange(64.0)[None])[0] == 2016.0


SETTINGS = [(nvar, f) for nvar in (4, 14, 40) for f in (0.0, 0.0005, 0.001, 0.003, 0.02)]


def test_the_interval_covers_the_planted_fraction():
    """The coverage simulation.  One generator, numpy.random.default_rng(26), for all fifteen settings in the order nvar = 4, 14, 40
    (outer) and f = 0, 0.0005, 0.001, 0.003, 0.02 (inner); a setting draws its 400 replicates at once, in this order:
        d = rng.integers(2500, 3501, (400, nvar, 2))                 reads per strand
        e = rng.uniform(0.0003, 0.001, (400, nvar, 2)) -> float32    the table's rates = the true background
        a = rng.uniform(0.2, 0.6, (400, nvar)) -> float32            the weights
        k = rng.binomial(d, e + f a)                                 the counts (e and a as doubles)
    Every setting must cover the planted f with its 95 % interval (F_LO <= f <= F_HI) in at least 0.92 of the replicates: the nominal
    0.95 less 2.75 binomial standard deviations of 400 draws.  Measured: 0.965 0.950 0.9575 0.9525 0.955 (nvar = 4), 0.9625 0.940
    0.9425 0.9475 0.970 (14), 0.9825 0.955 0.935 0.9525 0.9475 (40); the lower bound above zero in 3.5 % / 3.75 % / 1.75 % of the null
    samples and in 24.5 % / 66 % / 97 % at f = 0.0005; median F_HAT at nvar = 14 and 40: 0.000504 / 0.000500, 0.001016 / 0.000999,
    0.003026 / 0.003002, 0.019970 / 0.020041; at nvar = 4: 0.000444, 0.000936, 0.002970, 0.019996."""
    rng = np.random.default_rng(26)
    R = 400
    cover, above, median = {}, {}, {}
    for nvar, f in SETTINGS:
        d = rng.integers(2500, 3501, (R, nvar, 2))
        e = rng.uniform(0.0003, 0.001, (R, nvar, 2)).astype(np.float32)
        a = rng.uniform(0.2, 0.6, (R, nvar)).astype(np.float32)
        k = rng.binomial(d, e.astype(np.float64) + f * a.astype(np.float64)[:, :, None])
        est = fm.solve(fm.cells_from_counts(k, d, e, a))
        cover[nvar, f] = float(((est[:, fm.F_LO] <= f) & (f <= est[:, fm.F_HI])).mean())
        above[nvar, f] = float((est[:, fm.F_LO] > 0).mean())
        median[nvar, f] = float(np.median(est[:, fm.F_HAT]))
    for key in SETTINGS:
        print(key, "coverage", cover[key], "F_LO > 0", above[key], "median F_HAT", median[key])
    assert all(cover[key] >= 0.92 for key in SETTINGS), cover
    assert all(above[nvar, 0.0] <= 0.05 for nvar in (4, 14, 40))          # a null sample is seldom QUANTIFIED
    assert above[4, 0.0005] < above[14, 0.0005] < above[40, 0.0005] and above[40, 0.0005] > 0.9  # more variants, more power
    for nvar in (14, 40):
        for f in (0.0005, 0.001, 0.003, 0.02):
            assert abs(median[nvar, f] - f) <= 0.05 * f, (nvar, f, median[nvar, f])


def test_verdicts_and_changes_of_the_model():
    assert fm.verdict(4, 0.1, 0.05, 5) == fm.NOT_EVALUABLE and fm.verdict(5, 0.1, 0.05, 5) == fm.QUANTIFIED and fm.verdict(5, 0.1, 0.0, 5) == fm.BELOW
    assert fm.verdict(5, fm.NA, fm.NA, 0) == fm.NOT_EVALUABLE
    hi, lo = [0.003, 0.002, 0.004, 9.0], [0.001, 0.0005, 0.0015, 5.0]
    assert fm.change(fm.QUANTIFIED, hi, fm.QUANTIFIED, lo) == (fm.FALLING, 0.001 / 0.003) and fm.change(fm.QUANTIFIED, lo, fm.QUANTIFIED, hi)[0] == fm.RISING
    assert fm.change(fm.QUANTIFIED, hi, fm.BELOW, hi) == (fm.STABLE, 1.0) and fm.change(fm.NOT_EVALUABLE, hi, fm.BELOW, lo) == (fm.CHANGE_NOT_EVALUABLE, fm.NA)
    assert fm.change(fm.BELOW, [0.0, 0.0, 0.001, -1.0], fm.QUANTIFIED, hi) == (fm.RISING, fm.NA)
