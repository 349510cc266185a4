"""The host library's exports of the overdispersion arithmetic (ampli_host_overdispersion_cell_batch, ampli_host_nb_score_batch,
ampli_host_nb_tail: the text the kernels run, csrc/ampli_math.h) against the definition (tests/overdispersion_model.py).

The tolerance of Q is 1e-5: 3.9e-6 is half a float's spacing at Q <= 100 (2^-18), and 1e-6 relative on p is 4.4e-6 of Q.  The grid and
20 000 random quadruples are recorded with the model's Q (tests/golden/overdispersion/nb_grid.npz, written by python -m
tests.overdispersion_model); a sample of them is recomputed here, so that the record cannot drift from the model.

Measured (this file's prints): worst |Q - model| on the record 3.8e-6; omega within 0.11 of its bound.
Planted cohort (32 normals, 200 positions, 30 overdispersed cells at omega 1.5, 4 tumours, q_min 13), model | host:
  background at overdispersed cells passing Poisson 12 | 12, kept 1 | 1; ordinary background passing 0 | 0; variants on ordinary cells
  kept 16 of 16 | 16 of 16; on overdispersed cells passing Poisson 6 | 6, kept 3 | 3."""
import ctypes as C
import math
import os

import numpy as np

from amplisolve_amd import host_lib
from tests.dispersion_model import HIGH
from tests.helpers import GOLDEN
from tests.overdispersion_cohorts import planted_and_fit, stand_in_thr, tally
from tests.overdispersion_model import nb_q_exact, score_model

Q_TOL = 1e-5
MAX_TERMS = 1 << 20
PLANTED = dict(P=200, S=32, T=4)
Q_MIN = 13.0


def host_q(k, d, e, omega):
    k, d = np.ascontiguousarray(k, np.int32), np.ascontiguousarray(d, np.int32)
    e = np.ascontiguousarray(e, np.float32)
    w = None if omega is None else np.ascontiguousarray(omega, np.float64)
    q = np.full(len(k), np.nan, np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    assert host_lib().ampli_host_nb_score_batch(p(k), p(d), p(e), p(w), len(k), p(q)) == 0
    return q


def host_omega(status, n, K, D, x2, s2):
    a = [np.ascontiguousarray(status, np.uint8), np.ascontiguousarray(n, np.int32)] + [np.ascontiguousarray(v, np.float64) for v in (K, D, x2, s2)]
    out = np.full(len(a[0]), np.nan)
    host_lib().ampli_host_overdispersion_cell_batch(*[v.ctypes.data_as(C.c_void_p) for v in a], len(out), out.ctypes.data_as(C.c_void_p))
    return out


def _grid():
    return np.load(os.path.join(GOLDEN, "overdispersion", "nb_grid.npz"))


def test_q_on_the_recorded_grid():
    g = _grid()
    k, d, e, w, want = g["k"], g["d"], g["e"], g["omega"], g["q"]
    assert len(k) > 22000 and (w == 0).sum() > 3000 and w.max() == 1e4 and d.max() == 2 ** 31 - 1
    m = d.astype(np.float64) * np.where(e == 0, np.float32(0.0010008), e).astype(np.float64)
    assert m[e > 0].min() < 1.1e-3 and m.max() > 9.9e3 and k.max() >= 99999
    assert ((w > 0) & (w < 1e-8)).sum() > 100  # omega between 0 and 1e-8 holds the same tolerance
    got = host_q(k, d, e, w)
    exact = (want == -888) | (k == 0)  # a Q at the clamp is held to the tolerance: p may fall on either side of 1e-10
    assert np.array_equal(got[exact], want[exact].astype(np.float32)) and exact.sum() > 2000
    assert (e == -1).sum() == 18 and (want[e == -1] == -888).all() and (e == 0).sum() == 18
    near = (want > 99.0) & (want < 100)  # the clamp from below; from above it is exactly 100
    assert near.sum() >= 4 and (want == 100).sum() >= 8
    err = np.abs(got.astype(np.float64) - want)
    i = int(np.argmax(err))
    print(f"worst |Q - model| {err[i]:.3g} at k {k[i]} d {d[i]} e {e[i]} omega {w[i]} (Q {want[i]})")
    assert (err <= Q_TOL).all()


def test_the_record_is_the_models():
    g = _grid()
    rng = np.random.default_rng(1)
    cheap = np.nonzero(g["k"] < 400)[0]
    for i in rng.choice(cheap, 150, replace=False):
        assert float(nb_q_exact(g["k"][i], g["d"][i], g["e"][i], g["omega"][i])) == g["q"][i]


def test_omega_null_is_omega_zero():
    g = _grid()
    k, d, e = g["k"][:3000], g["d"][:3000], g["e"][:3000]
    assert host_q(k, d, e, None).tobytes() == host_q(k, d, e, np.zeros(3000)).tobytes()


def test_bad_omega_and_bad_arguments():
    q = host_q([5, 5, 5, 5, 0], [1000] * 5, [0.002] * 5, [-1e-300, float("nan"), float("inf"), -3.0, float("nan")])
    assert (q == np.float32(-1)).all()
    one = np.zeros(1, np.int32)
    f = np.zeros(1, np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    lib = host_lib()
    assert lib.ampli_host_nb_score_batch(None, p(one), p(f), None, 1, p(f)) == -1
    assert lib.ampli_host_nb_score_batch(p(one), p(one), p(f), None, 0, p(f)) == -1


def test_term_bound():
    """a sum never has more than 2^20 terms, an upward sum never more than AMPLI_NB_TERMS_UP(m, omega), a complement never more than k;
    a tail that does not fit is a NaN (and its score NA), not a wrong number"""
    lib = host_lib()
    t = C.c_int32(0)
    longest = 0
    for m in (1e-3, 0.5, 3.0, 40.0, 1e3, 1e4, 2.0e5):
        for w in (0.0, 1e-8, 1e-3, 0.3, 1.0, 1.5, 30.0, 1e4):
            up = 8 * math.sqrt(m + w * m * m) + 40 * (1 + m * w) + 64
            for k in {1, 2, int(m) + 1, int(m + 3 * math.sqrt(m + w * m * m)) + 1, int(10 * m) + 1, int(m + up) + 5}:
                p = lib.ampli_host_nb_tail(float(k), m, w, C.byref(t))
                longest = max(longest, t.value)
                assert t.value <= min(k, MAX_TERMS) + (up if k > m and up <= MAX_TERMS else 0) + 2, (k, m, w, t.value)
                assert t.value <= 2 * MAX_TERMS
                assert p != p or 0.0 <= p <= 1.0
    # first terms from 1e-250 down through the denormals to 0: no sum may start where its terms cannot fall any more
    for m, w in ((4.0, 0.0), (4.0, 0.3), (50.0, 0.0), (0.01, 0.0), (300.0, 1e-8)):
        for k in range(int(m) + 1, int(m) + 900):
            p = lib.ampli_host_nb_tail(float(k), m, w, C.byref(t))
            up = 8 * math.sqrt(m + w * m * m) + 40 * (1 + m * w) + 64  # a complement runs only where k is below this, then once upwards
            assert 0.0 <= p <= 1.0 and t.value <= min(k, up) + up + 2, (k, m, w, p, t.value)
        assert p == 0.0
    assert (host_q(np.arange(200, 300), [2000] * 100, [0.002] * 100, None) == 100).all()
    print("the longest tail:", longest, "terms")
    assert math.isnan(lib.ampli_host_nb_tail(3.0e6, 1e4, 1e4, C.byref(t))) and t.value == 0  # neither sum fits: refused before a term
    assert host_q([3000000], [2 ** 31 - 1], [np.float32(1e4 / (2 ** 31 - 1))], [1e4])[0] == np.float32(-1)


def test_planted_cohort_on_the_host():
    (normals, tumours, ref, over, variants), dm, s2, w_model, bound = planted_and_fit(**PLANTED)
    P = normals.shape[1]
    # every planted cell is HIGH on both strands and fitted near its omega; nothing else is fitted far from 0
    high = (dm["status"] & HIGH) != 0
    assert all(high[0, b, p] and high[1, b, p] for p, b in over)
    fitted = np.array([w_model[st, b, p] for p, b in over for st in range(2)])
    print("median fitted omega at the planted cells:", np.median(fitted), "HIGH cells:", int(high.sum()))
    assert 0.9 <= np.median(fitted) <= 1.8
    # the host's omega, fed the model's X2 and S2, within the forward bound; exactly 0 where the cell is not HIGH
    n8 = np.broadcast_to(dm["n"][None], (2, 4, P))
    w_host = host_omega(dm["status"].ravel(), n8.ravel(), dm["K"].ravel(), dm["D"].ravel(), dm["x2"].ravel(), s2.astype(np.float64).ravel()).reshape(2, 4, P)
    assert (w_host[~high] == 0).all() and (w_model[~high] == 0).all()
    print("omega: worst error over its bound", np.max(np.abs(w_host - w_model)[high] / bound[high]))
    assert (np.abs(w_host - w_model) <= bound).all()
    # both scores of every tumour cell, host against model
    thr = stand_in_thr(dm["K"].astype(np.float64), dm["D"].astype(np.float64))
    q0_m, _ = score_model(tumours, P, thr, None, ref, 100)
    q_m, _ = score_model(tumours, P, thr, w_model, ref, 100)
    T = tumours.shape[0]
    k = np.stack([tumours[:, :, 0:4], tumours[:, :, 4:8]], axis=-1)  # [T][P][4][2]
    d = np.broadcast_to(np.stack([tumours[:, :, 0:4].sum(-1), tumours[:, :, 4:8].sum(-1)], axis=-1)[:, :, None, :], k.shape)
    e = np.broadcast_to(np.transpose(thr, (2, 1, 0))[None], k.shape)
    ww = np.broadcast_to(np.transpose(w_host, (2, 1, 0))[None], k.shape)
    ev = q0_m != np.float32(-1)
    q0_h = np.where(ev, host_q(k.ravel(), d.ravel(), e.ravel(), None).reshape(k.shape), np.float32(-1))
    q_h = np.where(ev, host_q(k.ravel(), d.ravel(), e.ravel(), ww.ravel()).reshape(k.shape), np.float32(-1))
    assert ev.sum() == T * P * 6
    assert (np.abs(q0_h.astype(np.float64) - q0_m) <= Q_TOL).all() and (np.abs(q_h.astype(np.float64) - q_m) <= Q_TOL).all()
    tm, th = tally(q0_m, q_m, Q_MIN, over, variants), tally(q0_h, q_h, Q_MIN, over, variants)
    print("model", tm)
    print("host ", th)
    # the model's counts, measured before this test was written (the docstring); the host's may not exceed twice the model's
    assert tm["over_poisson"] == 12 and tm["over_kept"] == 1 and tm["ordinary_poisson"] == 0 and tm["ordinary_kept"] == 0
    assert th["over_kept"] <= 2 * tm["over_kept"] and th["ordinary_kept"] <= 2 * tm["ordinary_kept"] and th["over_poisson"] <= 2 * tm["over_poisson"]
    assert all(th["var_ordinary_kept"]) and len(th["var_ordinary_kept"]) == 16
    assert th["over_kept"] < th["over_poisson"]  # the correction removes background calls at the overdispersed cells
