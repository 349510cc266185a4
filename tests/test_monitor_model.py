"""The monitoring model's own parts (tests/monitor_model.py) against independent texts: its Poisson tail against the overdispersion
model's at omega = 0, the butterfly order against a literal 64-lane loop, the control draw against the dilution model's Philox, and
the rules of an evaluated entry one at a time.  No library, no GPU."""
import mpmath as mp
import numpy as np
import pytest

from tests import dilution_model as dm
from tests import monitor_model as mm
from tests.overdispersion_model import nb_tail


@pytest.mark.parametrize("lam", [1e-3, 0.1, 0.7, 1.0, 3.3, 10.0, 100.0, 1000.0])
def test_the_tail_equals_the_overdispersion_models_at_omega_zero(lam):
    for k in sorted({0, 1, 2, int(lam), int(lam) + 1, int(lam + 2 * lam ** 0.5) + 1, int(lam + 7 * lam ** 0.5) + 1, int(2 * lam) + 3}):
        a, b = mm.pois_tail(k, lam), nb_tail(k, lam, 0.0)
        with mp.workdps(mm.DPS):
            assert abs(a - b) <= mp.mpf(10) ** -28 * max(b, mp.mpf(10) ** -300), (k, lam)


def test_the_special_cases_of_the_score():
    assert mm.q_exact(1, 0, 5.0) == 0.0 and mm.q_exact(1, 3, 0.0) == 100.0 and mm.q_exact(0, 3, 1.0) == -1.0
    assert mm.q_exact(1, 1, 1e-12) == 100.0  # the clamp
    assert 0.0 < mm.q_exact(1, 12, 10.0) < mm.q_exact(1, 13, 10.0) < 100.0


def _literal_butterfly(x):
    """what 64 lanes do: every lane reads its partner's value of the step before, then adds"""
    x = [np.float64(v) for v in x]
    for off in (32, 16, 8, 4, 2, 1):
        x = [x[lane] + x[lane ^ off] for lane in range(64)]
    assert all(v.tobytes() == x[0].tobytes() for v in x)  # an IEEE addition is commutative: the lanes agree
    return x[0]


def test_the_butterfly_order():
    rng = np.random.default_rng(1)
    for scale in (1.0, 1e-8, 1e12):
        acc = rng.random(64) * scale * np.exp(rng.uniform(-20, 20, 64))
        got = mm.butterfly(acc)
        assert got.tobytes() == _literal_butterfly(acc).tobytes()
    acc = np.array([1e16] + [1.0] * 63)  # the order matters: lane by lane every 1 is lost, the butterfly pairs 62 of them first
    assert sum(acc) == 1e16 and mm.butterfly(acc) == 1e16 + 62
    assert mm.butterfly(np.zeros(64)).tobytes() == np.float64(0.0).tobytes()


def test_the_lanes_take_entries_in_ascending_order():
    """a list of 200 evaluated entries: lane j holds entries j, j + 64, j + 128 added in that order from +0.0"""
    P = 200
    rng = np.random.default_rng(2)
    thr = np.exp(rng.uniform(np.log(1e-4), np.log(1e-2), (2, 4, P))).astype(np.float32)
    ref = np.zeros(P, np.uint8)
    row = rng.integers(100, 60000, (P, 8)).astype(np.int64)
    ent = [(p, 1 + p % 3) for p in rng.permutation(P)]
    s, lf, lb = mm.entry_sums(row, P, thr, ref, ent, 100, 1000)
    assert s[mm.N_EVAL] == 200
    for st, got in ((0, lf), (1, lb)):
        lanes = []
        for j in range(64):
            a = np.float64(0.0)
            for i in range(j, 200, 64):
                p, y = ent[i]
                a = a + np.float64(int(row[p, 4 * st:4 * st + 4].sum())) * np.float64(thr[st, y, p])
            lanes.append(a)
        assert got.tobytes() == _literal_butterfly(lanes).tobytes()


def test_the_rules_of_an_evaluated_entry():
    P = 4
    thr = np.full((2, 4, P), 1e-3, np.float32)
    ref = np.array([0, 0, 4, 0], np.uint8)
    row = np.array([[500, 3, 0, 0, 400, 2, 0, 0]] * P, np.int64)

    def go(ent, cov=100, vaf=1000, thr=thr, row=row):
        return mm.entry_sums(row, P, thr, ref, ent, cov, vaf)

    s, lf, lb = go([(0, 1)])
    assert s == [1, 1, 3, 2, 503, 402] and lf == np.float64(503) * np.float64(np.float32(1e-3)) and lb == np.float64(402) * np.float64(np.float32(1e-3))
    assert go([(0, 1), (0, 1)])[0] == [2, 2, 6, 4, 1006, 804]      # a cell named twice counts twice
    assert go([(0, 2)])[0] == [1, 0, 0, 0, 503, 402]               # evaluated, not seen
    assert go([(0, 0)])[0][0] == 0 and go([(2, 1)])[0][0] == 0     # y == ref; no reference base
    assert go([(4, 1)])[0][0] == 0 and go([None, (1, 1)])[0][0] == 1  # p >= P; none
    assert go([(0, 1)], cov=403)[0][0] == 0 and go([(0, 1)], cov=402)[0][0] == 1
    for bad in (-1.0, np.nan, np.inf, -0.5):
        for st in range(2):
            t = thr.copy()
            t[st, 1, 0] = bad
            assert go([(0, 1)], thr=t)[0][0] == 0
    t = thr.copy()
    t[0, 1, 0] = 0.0
    assert go([(0, 1)], thr=t)[1] == np.float64(503) * np.float64(np.float32(0.0010008))
    absent = row.copy()
    absent[0, 0] = mm.ABSENT
    assert go([(0, 1)], row=absent)[0][0] == 0
    # the allele-fraction gate: 1000 * 5 <= pm * 905
    assert go([(0, 1)], vaf=6)[0][0] == 1 and go([(0, 1)], vaf=5)[0][0] == 0
    eq = np.array([[300, 100, 0, 0, 300, 100, 0, 0]] * P, np.int64)
    assert go([(0, 1)], vaf=250, row=eq)[0][0] == 1 and go([(0, 1)], vaf=249, row=eq)[0][0] == 0


def test_the_control_draw_is_the_dilution_models_philox():
    rng = np.random.default_rng(3)
    for _ in range(200):
        i, r, l, m = (int(rng.integers(0, 1 << 28)), int(rng.integers(0, 1 << 31)), int(rng.integers(0, 1 << 31)), int(rng.integers(1, 1 << 32)))
        seed = int(rng.integers(0, 1 << 63)) * 2 + int(rng.integers(0, 2))
        word = int(dm.philox(i, r, l, mm.TAG, seed & 0xFFFFFFFF, seed >> 32)[0])
        got = int(mm.control_draw(i, r, l, seed, m))
        assert got == (word * m) >> 32 and 0 <= got < m
    assert int(mm.control_draw(5, 6, 7, 8, 1)) == 0
    ctr, key, want = dm.KNOWN[2]
    assert tuple(int(w) for w in dm.philox(*ctr, *key)) == want


def test_a_control_list_keeps_the_base_and_the_reference_class():
    P = 300
    rng = np.random.default_rng(4)
    ref = rng.integers(0, 5, P).astype(np.uint8)
    cand_off, cand_pos = mm.candidates(ref)
    assert cand_off[4] == (ref <= 3).sum()
    ent = [(int(p), int(y)) for p, y in zip(rng.integers(0, P + 20, 150), rng.integers(0, 4, 150))]
    a = mm.control_entries(P, ref, ent, cand_off, cand_pos, 3, 17, 99)
    assert a == mm.control_entries(P, ref, ent, cand_off, cand_pos, 3, 17, 99) != mm.control_entries(P, ref, ent, cand_off, cand_pos, 3, 18, 99)
    for (p, y), c in zip(ent, a):
        if p >= P or ref[p] > 3:
            assert c is None
        else:
            assert c is not None and c[1] == y and ref[c[0]] == ref[p]
    empty = cand_off.copy()
    empty[1:] -= np.minimum(empty[1:], cand_off[1])  # no candidate of base 0
    b = mm.control_entries(P, ref, ent, empty, cand_pos[cand_off[1]:], 3, 17, 99)
    assert all(c is None for (p, y), c in zip(ent, b) if p < P and ref[p] == 0) and any(c is not None for c in b)


def test_verdicts_and_the_walk():
    assert mm.verdict(4, 9, 50, 50, 5, 1, 20.0) == mm.NOT_EVALUABLE and mm.verdict(5, 0, 50, 50, 5, 1, 20.0) == mm.NOT_DETECTED
    assert mm.verdict(5, 1, 20, 20, 5, 1, 20.0) == mm.DETECTED and mm.verdict(5, 1, np.float32(19.999), 20, 5, 1, 20.0) == mm.NOT_DETECTED
    assert mm.excess(10, 4.0, 1000) == 0.006 and mm.excess(3, 4.0, 1000) == 0.0 and mm.excess(3, 1.0, 0) == 0.0
    assert mm.empirical_p(0, 999) == 0.001 and mm.empirical_p(7, 7) == 1.0
    q = np.array([[30, 40], [10, 50], [25, 25], [-1, -1]], np.float32)
    assert mm.count_ge(25, 60, q) == 2 and mm.count_ge(-1, -1, q) == 4 and mm.count_ge(100, 100, q[:0]) == 0
    K, evals = mm.lod_reads(10.0, 20.0)
    assert mm.q_exact(1, K, 10.0) >= 20.0 > mm.q_exact(1, K - 1, 10.0) and evals == K - 10 and K == 19
    assert mm.lod_reads(10.0, 101.0) == (0, 0) and mm.lod_reads(0.0, 20.0)[0] == 1
    assert mm.lod(10.0, 2.5, 1000, 500, 20.0) == max((19 - 10.0) / 1000, (mm.lod_reads(2.5, 20.0)[0] - 2.5) / 500)
    assert mm.lod(10.0, 2.5, 0, 500, 20.0) == -1.0
