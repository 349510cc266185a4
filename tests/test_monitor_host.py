"""The host library's monitoring exports (ampli_host_monitor_*: csrc/ampli_math.h's text, the text the kernels run) against the model
(tests/monitor_model.py) without a GPU.  Integers and Lambda bit for bit -- the host runs the model's operations in the model's order;
the verdict arithmetic bit for bit; the pooled score within the project's 1e-5 of the 50-digit model on the recorded grid and on 20 000
recorded random sum vectors (tests/golden/monitor/pool_grid.npz, written by python -m tests.monitor_model)."""
import ctypes as C
import os

import numpy as np
import pytest

from amplisolve_amd import host_lib
from amplisolve_amd._lib import MonitorParams
from tests import monitor_model as mm
from tests.monitor_cases import CONTROL_SEED, COV, big_records, cohort, control_case, expected, lists, panel

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "monitor", "pool_grid.npz")
Q_BOUND = 1e-5  # the project's budget for a score


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def host_sums(recs, P, thr, ref, off, cell, cov=COV, vaf=1000, stride=0, W=None):
    n, L = recs.shape[0], len(off) - 1
    recs, cell = np.ascontiguousarray(recs, np.int32), np.ascontiguousarray(cell if len(cell) else np.zeros(1), np.uint32)
    sums, lam = np.full((n, L, 6), -1, np.int64), np.full((n, L, 2), np.nan)
    rc = host_lib().ampli_host_monitor_sums(_p(recs), n, stride, P, _p(np.ascontiguousarray(thr)), _p(np.ascontiguousarray(ref)),
                                            _p(np.ascontiguousarray(off, np.uint32)), _p(cell), L, len(cell) if W is None else W,
                                            C.byref(MonitorParams(cov, vaf)), _p(sums), _p(lam))
    return rc, sums, lam


def host_controls(recs, P, thr, ref, off, cell, pairs, cand_off, cand_pos, R, first_rep, seed, cov=COV, vaf=1000):
    n, L = recs.shape[0], len(off) - 1
    recs = np.ascontiguousarray(recs, np.int32)
    cp = np.ascontiguousarray(cand_pos if len(cand_pos) else np.zeros(1), np.uint32)
    sums, lam = np.full((len(pairs), R, 6), -1, np.int64), np.full((len(pairs), R, 2), np.nan)
    rc = host_lib().ampli_host_monitor_controls(_p(recs), n, 0, P, _p(np.ascontiguousarray(thr)), _p(np.ascontiguousarray(ref)),
                                                _p(np.ascontiguousarray(off, np.uint32)), _p(np.ascontiguousarray(cell, np.uint32)), L, len(cell),
                                                _p(np.ascontiguousarray(pairs, np.int32)), len(pairs), _p(np.ascontiguousarray(cand_off, np.uint32)), _p(cp),
                                                len(cand_pos), R, first_rep, seed, C.byref(MonitorParams(cov, vaf)), _p(sums), _p(lam))
    return rc, sums, lam


def host_score(sums, lam):
    sums, lam = np.ascontiguousarray(sums, np.int64).reshape(-1, 6), np.ascontiguousarray(lam, np.float64).reshape(-1, 2)
    q = np.full((len(sums), 2), np.nan, np.float32)
    assert host_lib().ampli_host_monitor_score(_p(sums), _p(lam), len(sums), _p(q)) == 0
    return q


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


@pytest.mark.parametrize("P,n", [(1, 1), (64, 3), (65, 9), (1000, 3)])
@pytest.mark.parametrize("vaf", [1000, 250])
def test_sums_equal_the_model(P, n, vaf):
    thr, ref = panel(P)
    off, cell = lists(P)
    exp_s, exp_l = expected(P, n, vaf)
    rc, sums, lam = host_sums(cohort(P, n), P, thr, ref, off, cell, vaf=vaf)
    assert rc == 0 and np.array_equal(sums, exp_s) and np.array_equal(bits(lam), bits(exp_l))
    if P >= 64:
        assert (exp_s[:, 1:8, mm.N_EVAL] > 0).any() and (exp_s[:, 9] == 0).all() and (exp_s[:, :, mm.N_SEEN] < exp_s[:, :, mm.N_EVAL]).any()


def test_the_gate_and_the_cut_off_change_the_sums():
    a, b, c = expected(65, 9, 1000)[0], expected(65, 9, 250)[0], sums_of_cov(65, 9, COV + 1)
    assert (a[:, :, mm.N_EVAL] > b[:, :, mm.N_EVAL]).any() and (a[:, :, mm.N_EVAL] > c[:, :, mm.N_EVAL]).any()


def sums_of_cov(P, n, cov):
    thr, ref = panel(P)
    off, cell = lists(P)
    rc, sums, lam = host_sums(cohort(P, n), P, thr, ref, off, cell, cov=cov)
    exp = mm.sums_model(cohort(P, n), P, thr, ref, off, cell, cov, 1000)
    assert rc == 0 and np.array_equal(sums, exp[0]) and np.array_equal(bits(lam), bits(exp[1]))
    return sums


def test_offsets_beyond_W_a_stride_and_deep_records():
    P, n = 65, 3
    thr, ref = panel(P)
    off, cell = lists(P)
    W = int(off[6]) + 10  # list 6 is cut, the later ones are empty
    exp = mm.sums_model(cohort(P, n), P, thr, ref, off, cell[:W], COV, 1000)
    rc, sums, lam = host_sums(cohort(P, n), P, thr, ref, off, cell, W=W)
    assert rc == 0 and np.array_equal(sums, exp[0]) and np.array_equal(bits(lam), bits(exp[1])) and (sums[:, 7:] == 0).all() and (sums[:, 6, 0] > 0).any()
    wide = cohort(P + 7, n)
    rc, sums, lam = host_sums(wide, P, thr, ref, off, cell, stride=P + 7)
    exp = mm.sums_model(wide[:, :P], P, thr, ref, off, cell, COV, 1000)
    assert rc == 0 and np.array_equal(sums, exp[0]) and np.array_equal(bits(lam), bits(exp[1]))
    deep = big_records(P, n)
    exp = mm.sums_model(deep, P, thr, ref, off, cell, COV, 1000)
    rc, sums, lam = host_sums(deep, P, thr, ref, off, cell)
    assert rc == 0 and np.array_equal(sums, exp[0]) and np.array_equal(bits(lam), bits(exp[1])) and (exp[0][:, :, mm.D_FW] > 1 << 36).any()


@pytest.mark.parametrize("kw", [dict(R=7), dict(R=3, first_rep=5), dict(R=2, empty_class=1), dict(R=2, single=True)])
def test_controls_equal_the_model(kw):
    P, n = 65, 3
    thr, ref = panel(P)
    off, cell = lists(P)
    pairs, cand_off, cand_pos, exp_s, exp_l = control_case(P, n, **kw)
    rc, sums, lam = host_controls(cohort(P, n), P, thr, ref, off, cell, pairs, cand_off, cand_pos, kw["R"], kw.get("first_rep", 0), CONTROL_SEED)
    assert rc == 0 and np.array_equal(sums, exp_s) and np.array_equal(bits(lam), bits(exp_l))
    assert (sums[9:] == 0).all() and (sums[:5, :, mm.N_EVAL] > 0).any()


def test_the_draw_equals_the_model():
    rng = np.random.default_rng(6)
    L = host_lib()
    for _ in range(2000):
        i, r, l, m = (int(rng.integers(0, 1 << 28)), int(rng.integers(0, 1 << 31)), int(rng.integers(0, 1 << 31)), int(rng.integers(1, 1 << 32)))
        seed = int(rng.integers(0, 1 << 63)) * 2 + int(rng.integers(0, 2))
        assert L.ampli_host_monitor_control_draw(i, r, l, seed, m) == int(mm.control_draw(i, r, l, seed, m))


def test_the_pooled_score_on_the_recorded_grid_and_random_vectors():
    g = np.load(GOLDEN)
    K, lam, q, n_grid = g["K"], g["lam"], g["q"], int(g["n_grid"])
    assert len(K) - n_grid == 20000 and lam[:n_grid].min() == 1e-3 and lam[:n_grid].max() == 1e6
    sums = np.zeros((len(K), 6), np.int64)
    sums[:, mm.N_EVAL], sums[:, mm.K_FW], sums[:, mm.K_BW] = 1, K, K[::-1]
    got = host_score(sums, np.stack([lam, lam[::-1]], 1))
    err = np.abs(got[:, 0].astype(np.float64) - q)
    assert err.max() <= Q_BOUND, (err.max(), K[err.argmax()], lam[err.argmax()])
    assert np.array_equal(got[:, 1], got[::-1, 0])  # a strand's score does not depend on the other strand
    assert ((q > 0) & (q < 100)).sum() > 5000 and (q == 100).any() and (q == 0).any()
    clamp = (q[:n_grid] > 99) & (q[:n_grid] < 100)  # the clamp approached from below, and reached
    assert clamp.any() and (got[:n_grid, 0][q[:n_grid] == 100] == 100).all()
    for i in np.nonzero(lam[:n_grid] >= 1e5)[0][::7]:  # the model itself, recomputed where the grid goes beyond DESIGN 19's 1e4
        assert mm.q_exact(1, K[i], lam[i]) == q[i]


def test_special_scores_and_verdict_arithmetic_on_random_vectors():
    rng = np.random.default_rng(8)
    n = 20000
    sums = rng.integers(0, 50, (n, 6)).astype(np.int64)
    sums[:, mm.D_FW:] = rng.integers(0, 1 << 34, (n, 2)) * (rng.random((n, 2)) < 0.9)
    lam = np.exp(rng.uniform(np.log(1e-3), np.log(1e3), (n, 2))) * (rng.random((n, 2)) < 0.9)
    q = host_score(sums, lam)
    none = sums[:, mm.N_EVAL] == 0
    assert none.any() and (q[none] == mm.NA).all() and (q[~none] >= 0).all() and (q <= 100).all()
    assert (q[~none & (sums[:, mm.K_FW] == 0), 0] == 0).all() and (q[~none & (sums[:, mm.K_BW] > 0) & (lam[:, 1] == 0), 1] == 100).all()
    L = host_lib()
    mv, ms, q_min = 5, 2, 20.0
    for i in range(0, n, 7):
        s = sums[i]
        assert L.ampli_host_monitor_verdict(int(s[0]), int(s[1]), q[i, 0], q[i, 1], mv, ms, q_min) == mm.verdict(s[0], s[1], q[i, 0], q[i, 1], mv, ms, q_min)
        for st in range(2):
            a, b = L.ampli_host_monitor_excess(int(s[mm.K_FW + st]), lam[i, st], int(s[mm.D_FW + st])), mm.excess(s[mm.K_FW + st], lam[i, st], s[mm.D_FW + st])
            assert np.float64(a).tobytes() == np.float64(b).tobytes()
    ctl = q[:999]
    for i in range(0, 2000, 13):
        n_ge = L.ampli_host_monitor_count_ge(q[i, 0], q[i, 1], _p(np.ascontiguousarray(ctl)), len(ctl))
        assert n_ge == mm.count_ge(q[i, 0], q[i, 1], ctl)
        assert L.ampli_host_monitor_empirical_p(n_ge, len(ctl)) == mm.empirical_p(n_ge, len(ctl))


def test_every_branch_of_the_verdict_and_equality():
    V = host_lib().ampli_host_monitor_verdict
    f = np.float32
    assert V(4, 4, f(50), f(50), 5, 1, 20.0) == mm.NOT_EVALUABLE and V(5, 4, f(50), f(50), 5, 1, 20.0) == mm.DETECTED  # N_EVAL at min_variants
    assert V(5, 0, f(50), f(50), 5, 1, 20.0) == mm.NOT_DETECTED and V(5, 1, f(50), f(50), 5, 1, 20.0) == mm.DETECTED   # N_SEEN at min_seen
    assert V(5, 1, f(20), f(20), 5, 1, 20.0) == mm.DETECTED                                                          # Q at q_min
    below = np.nextafter(f(20), f(0))
    assert V(5, 1, below, f(50), 5, 1, 20.0) == mm.NOT_DETECTED and V(5, 1, f(50), below, 5, 1, 20.0) == mm.NOT_DETECTED
    assert V(0, 0, f(-1), f(-1), 0, 0, 0.0) == mm.NOT_DETECTED and V(0, 0, f(-1), f(-1), 1, 0, 0.0) == mm.NOT_EVALUABLE  # NA is below every q_min >= 0
    E = host_lib().ampli_host_monitor_excess
    assert E(10, 4.0, 1000) == 0.006 and E(4, 4.0, 1000) == 0.0 and E(3, 4.0, 1000) == 0.0 and E(3, 1.0, 0) == 0.0 and E(3, 1.0, -5) == 0.0
    assert host_lib().ampli_host_monitor_empirical_p(0, 0) == 1.0 and host_lib().ampli_host_monitor_count_ge(f(1), f(1), None, 3) == -1


@pytest.mark.parametrize("lam", [0.0, 1e-3, 0.5, 2.5, 10.0, 99.99, 1000.0])
@pytest.mark.parametrize("q_min", [0.0, 13.0, 20.0, 60.0, 100.0])
def test_the_walk_of_the_limit_of_detection(lam, q_min):
    """the first K from floor(Lambda) + 1 whose Q reaches q_min; on the model no Q of the walk lies within 2e-5 of q_min (asserted), so
    the host's walk ends at the same count"""
    L = host_lib()
    K, evals = mm.lod_reads(lam, q_min)
    assert K > 0
    for k in (K - 1, K):
        assert k <= int(lam) or abs(mm.q_exact(1, k, lam) - q_min) > 2e-5 or mm.q_exact(1, k, lam) in (0.0, 100.0)
    e = C.c_int32(-1)
    assert L.ampli_host_monitor_lod_reads(lam, q_min, C.byref(e)) == K and e.value == evals == K - int(lam)
    got, want = L.ampli_host_monitor_lod(lam, 3.0, 5000, 700, q_min), mm.lod(lam, 3.0, 5000, 700, q_min)
    assert np.float64(got).tobytes() == np.float64(want).tobytes() and got > 0


def test_the_walk_gives_up_and_refuses():
    L = host_lib()
    e = C.c_int32(-1)
    assert L.ampli_host_monitor_lod_reads(1e6, 100.0, C.byref(e)) == 0 and e.value == mm.LOD_MAX_EVALS  # 6.4 sigma is 6400 counts away
    for lam, q_min in ((-1.0, 20.0), (np.nan, 20.0), (2.0 ** 52, 20.0), (5.0, 100.5), (5.0, np.nan)):
        assert L.ampli_host_monitor_lod_reads(lam, q_min, C.byref(e)) == 0 and e.value == 0
    assert L.ampli_host_monitor_lod_reads(5.0, 20.0, None) == mm.lod_reads(5.0, 20.0)[0]
    assert L.ampli_host_monitor_lod(5.0, 5.0, 0, 100, 20.0) == -1.0 and L.ampli_host_monitor_lod(5.0, 1e6, 100, 100, 100.0) == -1.0


def test_refusals_leave_the_outputs_untouched():
    P, n = 65, 3
    thr, ref = panel(P)
    off, cell = lists(P)
    recs = cohort(P, n)
    for kw, want in ((dict(cov=-1), -1), (dict(vaf=-1), -1), (dict(vaf=1001), -1), (dict(stride=P - 1), -1), (dict(W=-1), -1), (dict(W=1 << 28), -6)):
        rc, sums, lam = host_sums(recs, P, thr, ref, off, cell, **kw)
        assert rc == want and (sums == -1).all() and np.isnan(lam).all(), kw
    pairs, cand_off, cand_pos, _, _ = control_case(P, n, R=2)
    for first, want in ((-1, -1), ((1 << 31) - 2, -6)):
        rc, sums, lam = host_controls(recs, P, thr, ref, off, cell, pairs, cand_off, cand_pos, 2, first, 1)
        assert rc == want and (sums == -1).all() and np.isnan(lam).all()
    # R < 1 and n_pairs < 1 with every buffer valid: the count itself is what is refused
    sums, lam = np.full((len(pairs), 2, 6), -1, np.int64), np.full((len(pairs), 2, 2), np.nan)
    a = [np.ascontiguousarray(x) for x in (recs.astype(np.int32), thr, ref, off.astype(np.uint32), cell.astype(np.uint32), pairs, cand_off, cand_pos)]
    prm = MonitorParams(COV, 1000)
    for n_pairs, R in ((len(pairs), 0), (len(pairs), -1), (0, 2), (-1, 2)):
        rc = host_lib().ampli_host_monitor_controls(_p(a[0]), n, 0, P, _p(a[1]), _p(a[2]), _p(a[3]), _p(a[4]), len(off) - 1, len(cell), _p(a[5]), n_pairs, _p(a[6]),
                                                    _p(a[7]), len(cand_pos), R, 0, 1, C.byref(prm), _p(sums), _p(lam))
        assert rc == -1 and (sums == -1).all() and np.isnan(lam).all(), (n_pairs, R)
    assert host_lib().ampli_host_monitor_controls(_p(a[0]), n, 0, P, _p(a[1]), _p(a[2]), _p(a[3]), _p(a[4]), len(off) - 1, len(cell), _p(a[5]), len(pairs), _p(a[6]),
                                                  _p(a[7]), len(cand_pos), 2, 0, 1, C.byref(prm), _p(sums), _p(lam)) == 0 and (sums != -1).all()
    assert host_lib().ampli_host_monitor_score(None, None, 1, None) == -1
