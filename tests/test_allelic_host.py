"""The host library's allelic-imbalance exports (ampli_host_allelic_*: csrc/ampli_math.h's text, the text the kernels run) against the
model (tests/allelic_model.py) without a GPU.  Statuses, codes, (k_lo, m), v, signs and the integer addends are exact; |q| is within
the paired suite's S_TOL = 1e-5 of the model, whose tail shares nothing with ampli_math.h; the verdict's Q and imbalance are the model's
to 1e-9 (the same operations through the same libm)."""
import ctypes as C
import math

import numpy as np

from amplisolve_amd import host_lib
from amplisolve_amd._lib import AllelicParams
from tests import allelic_model as am

S_TOL = 1e-5  # tests/test_paired_host.py
MAX_M = 2 ** 31 - 1


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def host_batch(pair, present, k_lo, k_hi, cnt, lo, hi, min_depth=100, min_normals=5, half=True):
    n = len(pair)
    a = [np.ascontiguousarray(pair, np.int32), np.ascontiguousarray(present, np.uint8)] + [np.ascontiguousarray(x, np.int64) for x in (k_lo, k_hi, cnt, lo, hi)]
    q, km, v, code, terms = np.full(n, np.nan, np.float32), np.full((n, 2), -1, np.int32), np.full(n, np.nan), np.full(n, 255, np.uint8), np.full(n, -1, np.int32)
    rc = host_lib().ampli_host_allelic_site_batch(n, *[_p(x) for x in a], C.byref(AllelicParams(min_depth, min_normals, int(half))), _p(q), _p(km), _p(v),
                                                  _p(code), _p(terms))
    assert rc == 0
    return q, km, v, code, terms


def model_batch(pair, present, k_lo, k_hi, cnt, lo, hi, min_depth=100, min_normals=5, half=True):
    pair = np.asarray(pair, np.int8)
    pair = np.where((pair >= 0) & (pair < 6), pair, -1).astype(np.int8)  # anything that is not a pair code is "not het"
    k_lo, k_hi, cnt, lo, hi = (np.asarray(x, np.int64) for x in (k_lo, k_hi, cnt, lo, hi))
    st, v = am.cell_status(pair, np.asarray(present, bool), k_lo, k_hi, cnt, lo, hi, min_depth, min_normals, half)
    t = st >= am.TESTED_REF
    q = np.full(len(pair), am.NA, np.float32)
    km = np.zeros((len(pair), 2), np.int32)
    if t.any():
        q[t] = am.site_scores(k_lo[t], (k_lo + k_hi)[t], v[t])[0]
        km[t, 0], km[t, 1] = k_lo[t], (k_lo + k_hi)[t]
    code = (st.astype(np.int64) * 8 + np.where(pair >= 0, pair, am.NO_PAIR)).astype(np.uint8)
    return q, km, v, code


def check(args, **kw):
    q, km, v, code, terms = host_batch(*args, **kw)
    mq, mkm, mv, mcode = model_batch(*args, **kw)
    assert np.array_equal(code, mcode) and np.array_equal(km, mkm) and np.array_equal(v, mv)
    t = (code >> 3) >= am.TESTED_REF
    assert np.array_equal(q[~t], mq[~t]) and (q[~t] == am.NA).all()
    assert np.array_equal(np.sign(q[t]), np.sign(mq[t])) and not np.signbit(q[t][q[t] == 0]).any()
    err = np.abs(np.abs(q[t].astype(np.float64)) - np.abs(mq[t].astype(np.float64)))
    assert (err <= S_TOL).all(), err.max()
    assert (np.abs(q[t]) <= 100).all()
    return q, km, v, code, terms


def test_every_status_boundary():
    """each rule at equality and one read either side; the first rule that applies wins"""
    rows = []
    for pair in (-1, 0, 5, 6, 7):                       # not a pair code: NOT_HET whatever else holds
        rows.append((pair, 1, 60, 60, 9, 50, 50))
    rows.append((2, 0, 60, 60, 9, 50, 50))              # ABSENT before SHALLOW
    rows.append((2, 0, 1, 1, 9, 50, 50))
    for m in (99, 100, 101):                            # SHALLOW at min_depth = 100
        rows.append((1, 1, m // 2, m - m // 2, 9, 50, 50))
    for m in (MAX_M - 1, MAX_M, MAX_M + 1, 2 ** 33):    # DEEP beyond 2^31 - 1
        rows.append((3, 1, m // 2, m - m // 2, 9, 50, 50))
    for cnt in (4, 5, 6):                               # CNT at min_normals - 1, at equality, above
        rows.append((4, 1, 70, 60, cnt, 480, 520))
    for lo, hi in ((0, 9), (9, 0), (0, 0), (1, 1)):     # LO > 0 and HI > 0
        rows.append((0, 1, 70, 60, 9, lo, hi))
    cols = [np.array(c) for c in zip(*rows)]
    for half in (True, False):
        q, km, v, code, _ = check(cols, half=half)
        st = code >> 3
        assert st[:5].tolist() == [am.NOT_HET, am.TESTED_REF, am.TESTED_REF, am.NOT_HET, am.NOT_HET]
        assert st[5:7].tolist() == [am.ABSENT_REC] * 2
        assert st[7:10].tolist() == [am.SHALLOW, am.TESTED_REF, am.TESTED_REF]
        assert st[10:14].tolist() == [am.TESTED_REF, am.TESTED_REF, am.DEEP, am.DEEP]
        fb = am.TESTED_HALF if half else am.NO_REFERENCE
        assert st[14:17].tolist() == [fb, am.TESTED_REF, am.TESTED_REF]
        assert st[17:21].tolist() == [fb, fb, fb, am.TESTED_REF]
        assert v[15] == 480.0 / 1000.0 and (code[:5] & 7).tolist() == [7, 0, 5, 7, 7]


def test_score_edges():
    """k = 0, k = m, d == 0 (+0, never -0), p2 >= 1, the cap at 100, m = 2^31 - 1"""
    rows = [(0, 1, 0, 200, 9, 50, 50), (0, 1, 200, 0, 9, 50, 50),       # k = 0, k = m: capped at 100 on either side
            (0, 1, 100, 100, 9, 50, 50),                              # d == 0
            (0, 1, 101, 100, 9, 50, 50), (0, 1, 100, 101, 9, 50, 50),  # half a read off the mean: 2 p >= 1
            (0, 1, 0, 100, 9, 1, 10 ** 6), (0, 1, 100, 0, 9, 10 ** 6, 1),  # k = 0 where nearly nothing else is expected
            (0, 1, 30, 70, 9, 30, 70),                                # d == 0 with a share that is not a dyadic fraction
            (0, 1, MAX_M // 2, MAX_M - MAX_M // 2, 9, 50, 50), (0, 1, MAX_M // 2 + 40000, MAX_M - MAX_M // 2 - 40000, 9, 50, 50),
            (0, 1, MAX_M // 2 - 150000, MAX_M - MAX_M // 2 + 150000, 9, 50, 50), (0, 1, MAX_M, 0, 9, 50, 50), (0, 1, 0, MAX_M, 9, 2, 1)]
    q, km, v, code, terms = check([np.array(c) for c in zip(*rows)])
    assert q[0] == -100 and q[1] == 100
    assert q[2] == 0 and not np.signbit(q[2]) and q[3] == 0 and q[4] == 0 and not np.signbit(q[4])
    assert abs(q[5]) < 1 and abs(q[6]) < 1
    assert q[7] == 0 and not np.signbit(q[7])
    assert q[8] == 0 and 0 < q[9] < 100 and q[10] == -100 and q[11] == 100 and q[12] == -100
    assert km[8].tolist() == [MAX_M // 2, MAX_M] and terms[9] > 10000


def test_term_bound_over_a_grid():
    """a tail costs at most 8 sqrt(m v (1 - v)) + 64 terms, for every m < 2^31: from the mean outwards, at the cut-off, and beyond.  The
    whole grid is held against the bound; the model checks the scores of its shallower part and of a few of the deepest cells."""
    rows, var = [], []
    for m in (1, 2, 7, 100, 300, 2000, 65535, 1000003, 2 ** 22 + 1, 2 ** 30 + 3, MAX_M):
        for lo, hi in ((1, 1), (35, 65), (65, 35), (1, 99), (999, 1), (1, 10 ** 6)):
            v = lo / (lo + hi)
            sd = math.sqrt(m * v * (1 - v))
            for z in (-8, -6.5, -6, -3, -1, -0.01, 0.01, 1, 3, 6, 6.5, 8):
                k = min(m, max(0, int(round(m * v + z * sd))))
                rows.append((0, 1, k, m - k, 9, lo, hi))
                var.append(m * v * (1 - v))
    cols = [np.array(c) for c in zip(*rows)]
    q, km, v, code, terms = host_batch(*cols, min_depth=1)
    assert ((code >> 3) == am.TESTED_REF).all()
    assert (terms <= 8.0 * np.sqrt(np.array(var)) + 64.0).all() and np.array_equal(8.0 * np.sqrt(np.array(var)) + 64.0, am.term_bound(cols[2] + cols[3], v))
    assert terms.max() > 100000 and terms.max() < 1 << 19 and (q != am.NA).all()
    m = cols[2] + cols[3]
    deep = np.flatnonzero(m > am.LGAMMA_MAX_M)
    keep = np.concatenate([np.flatnonzero(m <= am.LGAMMA_MAX_M), deep[::7]])
    check([c[keep] for c in cols], min_depth=1)


def test_random_cells():
    rng = np.random.Generator(np.random.Philox(25))
    n = 20000
    m = np.exp(rng.uniform(0, math.log(2 ** 16), n)).astype(np.int64) + 1
    lo = rng.integers(0, 3000, n)
    hi = rng.integers(0, 3000, n)
    v = np.where((lo > 0) & (hi > 0), lo / np.maximum(lo + hi, 1), 0.5)
    k = np.clip(np.rint(m * v + rng.normal(0, 2.5, n) * np.sqrt(m * v * (1 - v) + 0.3)), 0, m).astype(np.int64)
    args = [rng.integers(-1, 7, n), rng.random(n) < 0.95, k, m - k, rng.integers(3, 8, n), lo, hi]
    for half in (True, False):
        q, km, v_, code, _ = check(args, min_depth=20, half=half)
        assert ((code >> 3) >= am.TESTED_REF).sum() > 5000
    # the addends of the region sums, integer for integer
    t = np.flatnonzero((code >> 3) >= am.TESTED_REF)[:3000]
    dev, q20 = am.site_sums(q[t], km[t], v_[t])
    a, b = C.c_int64(), C.c_int64()
    for i, j in enumerate(t):
        assert host_lib().ampli_host_allelic_site_sums(float(q[j]), int(km[j, 0]), int(km[j, 1]), float(v_[j]), C.byref(a), C.byref(b)) == 0
        assert (a.value, b.value) == (int(dev[i]), int(q20[i]))


def test_pair_export_on_all_bit_patterns():
    want = am.pair_codes(np.arange(64, dtype=np.uint8))
    assert [host_lib().ampli_host_allelic_pair(g) for g in range(64)] == want.tolist()
    assert host_lib().ampli_host_allelic_pair(0xFFFFFFC0 | 0b100111) == 0  # the bits above the six planes do not enter


def host_verdict(sums, min_sites, q_min, min_imb):
    s = np.ascontiguousarray(sums, np.int64)
    Q, imb = C.c_double(), C.c_double()
    v = host_lib().ampli_host_allelic_region_verdict(_p(s), min_sites, q_min, min_imb, C.byref(Q), C.byref(imb))
    return v, Q.value, imb.value


def test_region_verdict():
    rng = np.random.Generator(np.random.Philox(26))
    cases = [[2, 2, 4000, 3200, 2 * 100 << 20], [3, 3, 6000, 16 * 300, 3 * 100 << 20], [3, 0, 6000, 16 * 300, 0], [0, 0, 0, 0, 0], [1, 0, 100, 0, 0],
             [3, 1, 6000, 16 * 120 - 1, 60 << 20], [3, 1, 6000, 16 * 120, 60 << 20], [600, 40, 10 ** 6, 10 ** 5, 3000 << 20]]
    for _ in range(2000):
        s = int(rng.integers(0, 120))
        depth = int(s * rng.integers(100, 5000))
        cases.append([s, int(rng.integers(0, s + 1)), depth, int(depth * 16 * rng.uniform(0, 0.06)), int(s * rng.exponential(4.34) * (1 << 20))])
    seen = set()
    for c in cases:
        for min_sites, q_min, min_imb in ((3, 20.0, 0.02), (1, 13.0, 0.0), (0, 20.0, 0.02)):
            v, Q, imb = host_verdict(c, min_sites, q_min, min_imb)
            mv, mQ, mimb = am.region_verdict(c, min_sites, q_min, min_imb)
            assert v == mv, (c, Q, mQ)
            assert (math.isnan(Q) and math.isnan(mQ)) or abs(Q - mQ) <= 1e-9 * max(1.0, abs(mQ))
            assert (math.isnan(imb) and math.isnan(mimb)) or imb == mimb
            seen.add(v)
    assert seen == {am.FEW, am.BALANCED, am.IMBALANCED}
    assert host_verdict(cases[5], 3, 20.0, 0.02)[0] == am.BALANCED and host_verdict(cases[6], 3, 20.0, 0.02)[0] == am.IMBALANCED  # imbalance at equality
    assert host_lib().ampli_host_allelic_region_verdict(None, 3, 20.0, 0.02, None, None) == -1


def test_refusals():
    z = np.zeros(1, np.int64)
    out = [np.zeros(2, np.float32), np.zeros(2, np.int32), np.zeros(1), np.zeros(1, np.uint8)]
    for prm in (AllelicParams(0, 5, 1), AllelicParams(100, 0, 1), AllelicParams(100, 5, 2)):
        assert host_lib().ampli_host_allelic_site_batch(1, _p(np.zeros(1, np.int32)), _p(np.ones(1, np.uint8)), _p(z), _p(z), _p(z), _p(z), _p(z), C.byref(prm),
                                                        *[_p(o) for o in out], None) == -1
