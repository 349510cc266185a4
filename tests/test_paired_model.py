"""The definition of the paired comparison (tests/paired_model.py) against independent implementations: scipy's hypergeometric tails,
scipy's one-sided Fisher test on small tables, its own exact rationals where both of its paths apply, and the symmetry of the score.
The last test needs the export ampli_host_pair_score_batch; the others are model-only and pass on any tree that holds the model."""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
from scipy import stats

from amplisolve_amd import host_lib
from tests import paired_model as pm
from tests.paired_model import NA, hyper_tail, pair_s, pair_s_exact, score_model, support, verdict


def _tables(seed, count, d_max):
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < count:
        d_a, d_b = (int(v) for v in rng.integers(1, d_max + 1, 2))
        f = float(np.exp(rng.uniform(math.log(1e-3), math.log(0.9))))
        k_a, k_b = int(min(d_a, rng.binomial(d_a, f) + rng.integers(0, 4))), int(min(d_b, rng.binomial(d_b, min(1.0, f * rng.choice([0.2, 1.0, 3.0])))))
        out.append((k_a, d_a, k_b, d_b))
    return out


def test_tails_equal_scipy():
    """both tails of 400 random tables with depths up to 1000 and of corner tables up to 2^20: 1e-9 relative"""
    cases = _tables(1, 400, 1000) + [(30, 70000, 2, 65000), (1 << 10, 1 << 20, 900, 1 << 20), (5, 1 << 20, 0, 1000), (700, 1000, 1, 2), (40, 300000, 3, 300)]
    worst = 0.0
    for k_a, d_a, k_b, d_b in cases:
        N, K, n = d_a + d_b, k_a + k_b, d_a
        for up, ref in ((True, stats.hypergeom.sf(k_a - 1, N, K, n)), (False, stats.hypergeom.cdf(k_a, N, K, n))):
            p = float(pm.as_mpf(hyper_tail(N, K, n, k_a, up)))
            if ref > 1e-250:
                worst = max(worst, abs(p - ref) / ref)
                assert abs(p - ref) <= 1e-9 * ref, (k_a, d_a, k_b, d_b, up, p, ref)
    print("worst relative difference from scipy", worst)


def test_both_paths_of_the_model_agree(monkeypatch):
    """the rational path and the loggamma / fixed-point path on the same small tables: 1e-30"""
    cases = [c for c in _tables(2, 60, 140)]
    exact = [(c, up, hyper_tail(c[1] + c[3], c[0] + c[2], c[1], c[0], up)) for c in cases for up in (True, False)]
    assert all(isinstance(p, Fraction) for _, _, p in exact)
    monkeypatch.setattr(pm, "EXACT_MAX_N", 0)
    for (k_a, d_a, k_b, d_b), up, p in exact:
        q = hyper_tail(d_a + d_b, k_a + k_b, d_a, k_a, up)
        assert abs(q - pm.as_mpf(p)) <= pm.as_mpf(p) * pm.mp.mpf(10) ** -30


def test_scores_equal_fisher_exact_on_small_tables():
    n = 0
    for k_a, d_a, k_b, d_b in _tables(3, 300, 60):
        s = float(pair_s_exact(k_a, d_a, k_b, d_b))
        c = k_a * (d_a + d_b) - (k_a + k_b) * d_a
        if k_a + k_b == 0 or c == 0:
            assert s == 0.0
            continue
        table = [[k_a, d_a - k_a], [k_b, d_b - k_b]]
        p = stats.fisher_exact(table, alternative="greater" if c > 0 else "less")[1]
        want = -10 * math.log10(max(p, 1e-10))
        assert abs(abs(s) - want) <= 1e-8 and (s > 0) == (c > 0), (table, s, want)
        n += 1
    assert n > 200


def test_symmetry_zero_and_na():
    for k_a, d_a, k_b, d_b in _tables(4, 300, 5000) + [(3, 9, 3, 9), (5, 100, 50, 1000), (0, 50, 0, 70)]:
        s, t = pair_s(k_a, d_a, k_b, d_b), pair_s(k_b, d_b, k_a, d_a)
        c = k_a * d_b - k_b * d_a
        if c == 0 or k_a + k_b == 0:
            assert s == 0 and t == 0 and not np.signbit(s) and not np.signbit(t)
        else:
            assert s == -t and (s > 0) == (c > 0), (k_a, d_a, k_b, d_b, s, t)  # S(a, b) = -S(b, a): the same tail read from the other file
    assert pair_s(0, 1000, 900, 1000) == np.float32(-100) and pair_s(900, 1000, 0, 1000) == np.float32(100)
    lo, hi = support(10, 7, 6)
    assert (lo, hi) == (3, 6) and hyper_tail(10, 7, 6, 3, True) == 1
    # the evaluated mask: absent records, a strand below the cut-off in either file, a reference code beyond 3, the reference base, a bad row
    recs = np.zeros((2, 5, 8), np.int32)
    recs[:, :] = [90, 10, 0, 0, 95, 5, 0, 0]
    recs[1, 1, 0] = pm.ABSENT
    recs[0, 2, 4:] = [9, 0, 0, 0]
    ref = np.array([0, 0, 0, 7, 1], np.uint8)
    s, _ = score_model(recs, recs, 5, [(0, 1), (0, 2), (0, 0)], ref, 10)
    assert (s[1] == NA).all() and (s[0, 1:4] == NA).all() and (s[0, 0, 0] == NA).all() and (s[0, 0, 1:] == 0).all() and (s[0, 4, 1] == NA).all()
    assert (s[2, 2] == NA).all() and (s[2, 0, 1:] == 0).all()
    assert verdict(13.0, 13.5, 0.02, 0.0, 13.0, 0.005) == "HIGHER_IN_A" and verdict(-13.0, -20.0, 0.0, 0.02, 13.0, 0.005) == "LOWER_IN_A"
    assert verdict(13.0, 12.9, 0.5, 0.5, 13.0, 0.005) == "SHARED" and verdict(13.0, -13.0, 0.02, 0.001, 13.0, 0.005) == "UNRESOLVED"


def test_the_host_library_runs_the_definition():
    """the export this feature adds, on the tables of this file: 1e-5 on S, the sign exact (tests/test_paired_host.py holds the grid)"""
    t = _tables(5, 500, 100000)
    arr = [np.ascontiguousarray([c[j] for c in t], np.int32) for j in range(4)]
    s = np.full(len(t), np.nan, np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert host_lib().ampli_host_pair_score_batch(p(arr[0]), p(arr[1]), p(arr[2]), p(arr[3]), len(t), p(s)) == 0
    want = np.array([float(pair_s_exact(*c)) for c in t])
    assert (np.abs(s.astype(np.float64) - want) <= 1e-5).all() and np.array_equal(np.sign(s), np.sign(want))
