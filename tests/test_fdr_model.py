"""The model of false-discovery control (tests/fdr_model.py) against scipy's Benjamini-Hochberg and against the definition word for
word, and the key rules one by one."""
import numpy as np
import pytest

from tests import fdr_model as fm


def _random_row(rng, n, two_sided):
    """heavy ties, zeros, clamped hundreds, NA cells"""
    a = rng.choice(np.array([0.0, 0.0, 1.5, 3.0, 7.25, 13.0, 13.0, 20.5, 55.0, 100.0, 100.0]), n)
    a = np.where(rng.random(n) < 0.4, np.round(rng.exponential(9.0, n), 1), a)
    a = np.minimum(a, 100.0).astype(np.float32).astype(np.float64)
    cls = np.where(a > 0, fm.PLUS, fm.ZERO)
    if two_sided:
        cls = np.where((a > 0) & (rng.random(n) < 0.5), fm.MINUS, cls)
    na = rng.random(n) < 0.15
    return np.where(na, 0.0, a), np.where(na, fm.UNTESTED, cls)


def test_the_model_is_scipys_benjamini_hochberg():
    """p = 10^(-a / 10) of the tested cells of 200 random rows of 1 to 400 cells: A = -10 log10(q_BH) to 1e-9, q clipped at 1"""
    from scipy.stats import false_discovery_control

    rng = np.random.default_rng(2026)
    worst, rows = 0.0, 0
    for _ in range(200):
        n = int(rng.integers(1, 401))
        a, cls = _random_row(rng, n, False)
        out, m, R = fm.adjust_row(a, cls, False)
        tested = cls != fm.UNTESTED
        assert m == tested.sum()
        if m == 0:
            assert (out == fm.NA).all()
            continue
        q = false_discovery_control(10.0 ** (-a[tested] / 10.0), method="bh")
        want = np.maximum(0.0, -10.0 * np.log10(q))
        pos = a[tested] > 0
        worst = max(worst, float(np.abs(out[tested][pos] - want[pos]).max()) if pos.any() else 0.0)
        assert (out[tested][~pos] == 0).all()
        rows += 1
    print("rows", rows, "worst |A - scipy|", worst)
    assert rows >= 150 and worst <= 1e-9


def test_the_two_sided_model_is_benjamini_hochberg_of_doubled_p_values():
    from scipy.stats import false_discovery_control

    rng = np.random.default_rng(7)
    for _ in range(100):
        n = int(rng.integers(1, 300))
        a, cls = _random_row(rng, n, True)
        out, m, R = fm.adjust_row(a, cls, True)
        tested = cls != fm.UNTESTED
        if m == 0:
            continue
        # scipy refuses p > 1.  Clipping the doubled p at 1 changes no q: a term m p_j / j with p_j >= 1 is at least 1 either way
        # (j <= m), and q is clipped at 1
        p2 = np.minimum(2.0 * 10.0 ** (-a[tested] / 10.0), 1.0)
        want = np.maximum(0.0, -10.0 * np.log10(false_discovery_control(p2, method="bh")))
        pos = a[tested] > 0
        got = out[tested]
        assert (np.abs(np.abs(got[pos]) - want[pos]) <= 1e-9).all() and (got[~pos] == 0).all()
        neg = cls[tested] == fm.MINUS
        assert (got[neg] <= 0).all() and (got[~neg] >= 0).all()


@pytest.mark.parametrize("two_sided", [False, True])
def test_the_model_is_the_definition_word_for_word(two_sided):
    rng = np.random.default_rng(11 + two_sided)
    for _ in range(150):
        n = int(rng.integers(1, 61))
        a, cls = _random_row(rng, n, two_sided)
        out, m, R = fm.adjust_row(a, cls, two_sided)
        out_l, m_l, R_l = fm.adjust_row_literal(a, cls, two_sided)
        assert m == m_l and np.array_equal(R, R_l)
        assert np.array_equal(out == fm.NA, out_l == fm.NA) and np.abs(out - out_l).max() <= 1e-12
        assert not (np.signbit(out) & (out == 0)).any()


def _cell(f, b, two_sided):
    a, cls = fm.keys(np.array([[[f, b]]], np.float32), two_sided)
    return float(a[0, 0]), int(cls[0, 0])


@pytest.mark.parametrize("two_sided", [False, True])
def test_key_rules(two_sided):
    U, Z, PL, MI = fm.UNTESTED, fm.ZERO, fm.PLUS, fm.MINUS
    for na in (-888.0, -999.0):
        for other in (na, 5.0, 0.0, -3.0):
            assert _cell(na, other, two_sided) == (0.0, U) and _cell(other, na, two_sided) == (0.0, U)
    # -1, the negative-binomial plane's NA, is untested there and an ordinary score of the two-sided plane
    assert _cell(-1.0, -1.0, two_sided) == ((1.0, MI) if two_sided else (0.0, U))
    assert _cell(-1.0, 5.0, two_sided) == ((0.0, Z) if two_sided else (0.0, U))
    assert _cell(0.0, -1.0, two_sided) == ((0.0, Z) if two_sided else (0.0, U))
    for bad in (np.nan, np.inf, -np.inf, 100.0001, -100.0001):
        assert _cell(bad, 5.0, two_sided) == (0.0, U) and _cell(5.0, bad, two_sided) == (0.0, U)
    assert _cell(100.0, 100.0, two_sided) == (100.0, PL)
    assert _cell(-0.0, 7.0, two_sided) == (0.0, Z) and _cell(7.0, -0.0, two_sided) == (0.0, Z) and _cell(-0.0, -0.0, two_sided) == (0.0, Z)
    assert _cell(3.0, 7.0, two_sided) == (3.0, PL) and _cell(7.0, 3.0, two_sided) == (3.0, PL)
    # strands of mixed sign
    assert _cell(3.0, -7.0, two_sided) == ((0.0, Z) if two_sided else (0.0, U))
    assert _cell(-3.0, -7.0, two_sided) == ((3.0, MI) if two_sided else (0.0, U))
    assert _cell(-100.0, -100.0, two_sided) == ((100.0, MI) if two_sided else (0.0, U))


def test_a_single_tested_cell_keeps_its_key_and_the_sign():
    s = np.full((1, 5, 4, 2), -999.0, np.float32)
    s[0, 2, 1] = (17.25, 30.0)
    A, m, R = fm.adjust(s, False)
    assert m[0] == 1 and A[0, 2, 1] == 17.25 and R[0, 2, 1] == 1 and (A == fm.NA).sum() == 19
    s[0, 2, 1] = (-17.25, -30.0)
    A, m, R = fm.adjust(s, True)
    assert m[0] == 1 and abs(A[0, 2, 1] + (17.25 - 10 * np.log10(2.0))) < 1e-12
