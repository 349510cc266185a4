"""The host library's exports of the paired comparison's arithmetic (ampli_host_pair_score_batch, ampli_host_hyper_tail: the text the
kernel runs, csrc/ampli_math.h) against the definition (tests/paired_model.py).

The tolerance of S is 1e-5, the project's budget from DESIGN 19: 3.9e-6 is half a float's spacing at |S| <= 100 (2^-18), and a 1e-6
relative budget on p is 4.4e-6 of S.  The grid -- k_a in {0, 1, 2, around the mean, both ends of the support} x depths 1 .. 2^31 - 1,
balanced and 1000 : 1 x K from 0 to N, the 1e-10 clamp from both sides and on both signs, c == 0, K == 0 and 20 000 random tables -- is
recorded with the model's S (tests/golden/paired/hyper_grid.npz, written by python -m tests.paired_model); a sample of it is recomputed
here, so that the record cannot drift from the model.  The sign, NA, +0 and +-100 are exact.

Measured (this file's prints): 20 891 cases, worst |S - model| 3.8e-6 (at |S| = 79.7: the float's own rounding); worst relative error
of p 9.8e-10; the longest sum 100 163 terms of a bound of 131 136 (depths 2^31 - 1, K = N / 2)."""
import ctypes as C
import math
import os

import numpy as np

from amplisolve_amd import host_lib
from tests.helpers import GOLDEN
from tests.paired_model import D_MAX, as_mpf, hyper_tail, hyper_variance, pair_s_exact

S_TOL = 1e-5
MAX_TERMS = 1 << 20
_p = lambda a: a.ctypes.data_as(C.c_void_p)


def host_s(k_a, d_a, k_b, d_b):
    a = [np.ascontiguousarray(v, np.int32) for v in (k_a, d_a, k_b, d_b)]
    s = np.full(len(a[0]), np.nan, np.float32)
    assert host_lib().ampli_host_pair_score_batch(_p(a[0]), _p(a[1]), _p(a[2]), _p(a[3]), len(s), _p(s)) == 0
    return s


def _grid():
    g = np.load(os.path.join(GOLDEN, "paired", "hyper_grid.npz"))
    return g["k_a"], g["d_a"], g["k_b"], g["d_b"], g["s"]


def test_s_on_the_recorded_grid():
    k_a, d_a, k_b, d_b, want = _grid()
    assert len(want) > 20800 and d_a.max() == D_MAX and d_b.max() == D_MAX and d_a.min() == 1 and d_b.min() == 1
    ratio = d_a.astype(np.float64) / d_b
    assert (ratio >= 999).sum() > 100 and (ratio <= 1 / 999).sum() > 100 and (ratio == 1).sum() > 100
    K, N = k_a.astype(np.int64) + k_b, d_a.astype(np.int64) + d_b
    c = k_a.astype(np.int64) * d_b - k_b.astype(np.int64) * d_a
    assert (K == 0).sum() > 20 and (K == N).sum() > 20 and ((c == 0) & (K > 0) & (K < N)).sum() >= 3
    got = host_s(k_a, d_a, k_b, d_b)
    # exact: the sign, +0 (K == 0, c == 0) without a sign bit, +-100 beyond the clamp
    assert np.array_equal(np.sign(got), np.sign(c).astype(np.float32)) and np.array_equal(np.sign(want), np.sign(c).astype(np.float64))
    assert not np.signbit(got[got == 0]).any() and (got[(K == 0) | (c == 0)] == 0).all()
    clamped = np.abs(want) == 100
    near = (np.abs(want) > 99.0) & ~clamped
    assert clamped.sum() > 100 and near.sum() >= 8 and (want[near] > 0).any() and (want[near] < 0).any()
    assert (want == 100).sum() > 20 and (want == -100).sum() > 20
    assert np.array_equal(np.abs(got) == 100, clamped)  # no p of the grid lies within 1e-6 of 1e-10, where it could fall on either side
    err = np.abs(got.astype(np.float64) - want)
    i = int(np.argmax(err))
    print(f"{len(want)} cases, worst |S - model| {err[i]:.3g} at k_a {k_a[i]} d_a {d_a[i]} k_b {k_b[i]} d_b {d_b[i]} (S {want[i]})")
    assert (err <= S_TOL).all()
    assert not (got == np.float32(-999)).any()


def test_the_record_is_the_models():
    k_a, d_a, k_b, d_b, want = _grid()
    rng = np.random.default_rng(1)
    cheap = np.nonzero(hyper_variance(k_a, d_a, k_b, d_b) < 1e5)[0]
    for i in rng.choice(cheap, 300, replace=False):
        assert float(pair_s_exact(k_a[i], d_a[i], k_b[i], d_b[i])) == want[i]


def test_tail_and_term_bound_on_every_grid_case():
    """p itself to 1e-6 relative on a sample (measured: 1e-9), and on EVERY case of the grid: no sum longer than AMPLI_HYPER_TERMS(var) =
    8 sqrt(var) + 64 terms, var the hypergeometric variance, and none near the loop's own bound of 2^20"""
    k_a, d_a, k_b, d_b, want = _grid()
    lib = host_lib()
    t = C.c_int32(0)
    K, N = k_a.astype(np.int64) + k_b, d_a.astype(np.int64) + d_b
    c = k_a.astype(np.int64) * d_b - k_b.astype(np.int64) * d_a
    bound = 8.0 * np.sqrt(hyper_variance(k_a, d_a, k_b, d_b)) + 64.0
    assert bound.max() < MAX_TERMS / 4  # 8 sqrt(2^28) + 64: no int32 table comes near the loop's bound
    longest, at, worst = 0, 0, 0.0
    rng = np.random.default_rng(2)
    sample = set(rng.choice(len(want), 400, replace=False).tolist())
    for i in np.nonzero((c != 0) & (K > 0))[0]:
        p = lib.ampli_host_hyper_tail(int(N[i]), int(K[i]), int(d_a[i]), int(k_a[i]), 1 if c[i] > 0 else 0, C.byref(t))
        assert 0.0 <= p <= 1.0 and 1 <= t.value <= bound[i], (i, p, t.value, bound[i])
        if t.value > longest:
            longest, at = t.value, i
        if i in sample and bound[i] < 3000 and p > 0:
            e = float(as_mpf(hyper_tail(int(N[i]), int(K[i]), int(d_a[i]), int(k_a[i]), bool(c[i] > 0))))
            worst = max(worst, abs(p - e) / e)
        if p == 0.0:
            assert abs(want[i]) == 100 and t.value == 1  # decided by the first term alone
    print(f"the longest sum: {longest} terms of a bound of {bound[at]:.0f} (k_a {k_a[at]} d_a {d_a[at]} k_b {k_b[at]} d_b {d_b[at]}); worst relative error of p {worst:.3g}")
    assert worst <= 1e-6 and longest > 50000
    # the prototype's longest sum below the clamp: 2 728 terms
    p = lib.ampli_host_hyper_tail(2 * D_MAX, (1 << 21) + 5000, D_MAX, (1 << 20) + 5000, 1, C.byref(t))
    assert t.value == 2728 and abs(p - 2.816282083768092e-4) < 1e-12


def test_arguments():
    lib = host_lib()
    t = C.c_int32(7)
    for N, K, n, k in ((10, 3, 0, 0), (10, 3, 10, 3), (10, 11, 5, 2), (10, 3, 5, 4), (10, 8, 5, 2), (1, 0, 0, 0)):
        assert math.isnan(lib.ampli_host_hyper_tail(N, K, n, k, 1, C.byref(t))) and t.value == 0
    assert lib.ampli_host_hyper_tail(10, 7, 6, 3, 1, None) == 1.0  # from the near side of the mean: the sum runs away from it only
    one, s = np.zeros(1, np.int32), np.full(1, 5.0, np.float32)
    assert lib.ampli_host_pair_score_batch(None, _p(one), _p(one), _p(one), 1, _p(s)) == -1
    assert lib.ampli_host_pair_score_batch(_p(one), _p(one), _p(one), _p(one), 0, _p(s)) == -1
    bad = np.array([3], np.int32)
    assert lib.ampli_host_pair_score_batch(_p(bad), _p(one), _p(one), _p(one), 1, _p(s)) == -1 and s[0] == 5.0  # k_a > d_a: nothing written
    # depths of zero are legal (depth_cutoff 0): c == 0
    assert host_s([0, 0, 0], [0, 0, 5], [0, 2, 0], [0, 9, 0]).tolist() == [0.0, 0.0, 0.0]
