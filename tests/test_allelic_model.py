"""The allelic-imbalance model (tests/allelic_model.py) on the planted cohort of tests/allelic_cohorts.py: what the statistic
finds and what it leaves alone, checked on the model before anything relies on it.  No GPU, no library.

Why no (normal, gene) may be flagged at depths of 1500 .. 2500: a region is IMBALANCED only with Q >= 20 AND a pooled deviation of the
share of at least 0.02.  Under binomial reads the deviation of one site has a standard deviation of at most 0.5 / sqrt(1500) = 0.013
and a mean absolute value of 0.8 of that, so the depth-weighted mean over three or more sites reaches 0.02 only far out in its tail,
and the normals count in their own reference, which pulls them towards it."""
import math

import numpy as np
import pytest

from . import allelic_cohorts as ac
from . import allelic_model as am
from . import concordance_model as cm


@pytest.fixture(scope="module")
def run():
    co = ac.planted()
    return co, ac.run_model(co)


def test_cohort_shape(run):
    co, out = run
    assert co["normals"].shape == (24, 600, 8) and co["tumours"].shape == (6, 600, 8)
    het = am.pair_codes(cm.classify(co["normals"])) >= 0
    assert 0.10 < het.mean() < 0.20
    assert 0.35 <= co["share"].min() and co["share"].max() <= 0.65
    tested = (out["tumours"]["code"] >> 3) >= am.TESTED_REF
    assert tested.sum() > 300 and ((out["tumours"]["code"] >> 3) == am.TESTED_HALF).sum() < tested.sum()


def test_planted_gene_is_imbalanced(run):
    co, out = run
    t, g = co["plant"]
    verdict, Q, imb = out["tumours"]["verdicts"][t][g]
    assert verdict == am.IMBALANCED and Q >= 20.0 and imb >= 0.02
    # and it is the only gene of any tumour that is
    flagged = [(s, r) for s in range(6) for r in range(ac.GENES) if out["tumours"]["verdicts"][s][r][0] == am.IMBALANCED]
    assert flagged == [(t, g)]


def test_no_normal_gene_is_imbalanced(run):
    _, out = run
    v = out["normals"]["verdicts"]
    flagged = [(s, r) for s in range(len(v)) for r in range(len(v[s])) if v[s][r][0] == am.IMBALANCED]
    assert flagged == []
    assert sum(1 for row in v for x in row if x[0] == am.BALANCED) > 200  # the cap is met by tested regions, not by FEW ones


def test_no_site_score_at_the_gate(run):
    _, out = run
    for key in ("tumours", "normals"):
        q64 = out[key]["q64"]
        tested = (out[key]["code"] >> 3) >= am.TESTED_REF
        assert (np.abs(np.abs(q64[tested]) - am.DEFAULTS["site_q"]) > 1e-3).all()


def test_reference_share_tracks_the_bias(run):
    co, out = run
    ref = out["ref"]
    ok = (ref[0] >= 5) & (ref[1] > 0) & (ref[2] > 0)
    c, p = np.nonzero(ok)
    share = ref[1][c, p] / (ref[1][c, p] + ref[2][c, p])
    assert len(p) > 100 and np.abs(share - co["share"][p]).max() < 0.02


def test_status_order_and_codes():
    codes = np.array([-1, 0, 1, 2, 3, 4, 5, 5], np.int8)
    present = np.array([1, 0, 1, 1, 1, 1, 1, 1], bool)
    k_lo = np.array([50, 50, 49, 2 ** 31, 60, 60, 60, 60], np.int64)
    k_hi = np.array([50, 50, 50, 0, 60, 60, 60, 60], np.int64)
    cnt = np.array([9, 9, 9, 9, 4, 5, 5, 5], np.int64)
    lo = np.array([5, 5, 5, 5, 5, 5, 0, 7], np.int64)
    hi = np.array([5, 5, 5, 5, 5, 5, 9, 0], np.int64)
    st, v = am.cell_status(codes, present, k_lo, k_hi, cnt, lo, hi, 100, 5, False)
    assert st.tolist() == [am.NOT_HET, am.ABSENT_REC, am.SHALLOW, am.DEEP, am.NO_REFERENCE, am.TESTED_REF, am.NO_REFERENCE, am.NO_REFERENCE]
    assert v.tolist() == [0, 0, 0, 0, 0, 0.5, 0, 0]
    st, v = am.cell_status(codes, present, k_lo, k_hi, cnt, lo, hi, 100, 5, True)
    assert st.tolist()[4:] == [am.TESTED_HALF, am.TESTED_REF, am.TESTED_HALF, am.TESTED_HALF] and v.tolist()[4:] == [0.5, 0.5, 0.5, 0.5]


def test_pair_codes_of_all_64_bit_patterns():
    got = am.pair_codes(np.arange(64, dtype=np.uint8))
    for g in range(64):
        bases = [b for b in range(4) if g >> (b + 1) & 1]
        want = am.PAIRS.index(tuple(bases)) if (g & 1 and g & 32 and len(bases) == 2) else -1
        assert got[g] == want


def test_tail_against_exact_rationals():
    from fractions import Fraction

    for m, k, v in ((10, 7, 0.5), (30, 4, 0.4), (100, 61, 0.5), (100, 100, 0.37), (100, 0, 0.63), (257, 120, 0.55)):
        q, q64 = am.site_scores(np.array([k]), np.array([m]), np.array([v]))
        V = Fraction(v)
        pm = [math.comb(m, x) * V ** x * (1 - V) ** (m - x) for x in range(m + 1)]
        d = k - v * m
        p = sum(pm[k:]) if d > 0 else sum(pm[:k + 1])
        want = 0.0 if 2 * p >= 1 else -10 * math.log10(max(float(2 * p), 1e-10))
        assert abs(abs(q64[0]) - want) < 1e-9 and (q64[0] >= 0) == (d > 0 or want == 0)
        assert q[0] == np.float32(q64[0])


def test_verdict_fractions():
    assert am.fraction_cnloh(0.05) == 0.1
    f = am.fraction_loss(0.05)
    assert abs(f / (2 * (2 - f)) - 0.05) < 1e-15  # a tumour fraction f with one copy lost moves the share by f / (2 (2 - f))
    assert am.region_verdict([2, 2, 4000, 3200, 2 * 100 << 20], 3)[0] == am.FEW
    v, Q, imb = am.region_verdict([3, 3, 6000, 16 * 300, 3 * 100 << 20], 3)
    assert v == am.IMBALANCED and Q > 100 and imb == 0.05
    assert am.region_verdict([3, 0, 6000, 16 * 300, 0], 3)[:2] == (am.BALANCED, 0.0)
