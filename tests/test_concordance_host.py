"""ampli_host_genotype_classify_batch and ampli_host_concordance_relation (csrc/ampli_math.h: the text the kernels run, compiled for
the host) against the definition in tests/concordance_model.py, exactly: every bound of the definition at equality and one read either
side, the depth gate, three and four het bases, absent and all-zero records, counts at 65 534 and at 2^30 per field, where a 32-bit
product wraps, and 20 000 random records; the relation on its three branches and at equality; bad parameter sets refused."""
import ctypes as C

import numpy as np
import pytest

from amplisolve_amd import host_lib
from amplisolve_amd._lib import GenotypeParams
from tests.concordance_cohorts import boundary_grid, random_records
from tests.concordance_model import ABSENT, DEFAULTS, DIFFERENT, H, SAME, UNDETERMINED, V, classify, relation

E_INVALID = -1


def _host(recs, **prm):
    recs = np.ascontiguousarray(recs, np.int32)
    bits = np.full(len(recs), 0xEE, np.uint8)
    q = GenotypeParams(*[dict(DEFAULTS, **prm)[k] for k in DEFAULTS])
    rc = host_lib().ampli_host_genotype_classify_batch(recs.ctypes.data_as(C.c_void_p), len(recs), C.byref(q), bits.ctypes.data_as(C.c_void_p))
    return rc, bits


def test_boundary_grid_equals_the_model():
    grid = boundary_grid()
    rc, got = _host(grid)
    exp = classify(grid)
    assert rc == 0 and np.array_equal(got, exp)
    assert (exp != 0).sum() >= 100 and (exp == 0).sum() >= 100 and ((exp & H) != 0).sum() >= 30  # the grid has both sides of the bounds
    # a few of its records by hand
    by_hand = {(450, 50, 0, 0, 450, 50, 0, 0): V | 2, (450, 50, 0, 0, 450, 51, 0, 0): 0, (125, 375, 0, 0, 125, 375, 0, 0): V | H | 2 | 4,
               (124, 376, 0, 0, 125, 375, 0, 0): 0, (100, 0, 0, 0, 0, 0, 0, 0): V | 2, (99, 0, 0, 0, 0, 0, 0, 0): 0,
               (250, 250, 250, 250, 0, 0, 0, 0): 0, (250, 250, 500, 0, 0, 0, 0, 0): 0, (0,) * 8: 0, (ABSENT, 500, 0, 0, 500, 0, 0, 0): 0,
               (1 << 30,) * 8: 0, (1 << 30, 0, 0, 0, 1 << 30, 0, 0, 0): V | 2, (9 << 27, 1 << 27, 0, 0, 0, 0, 0, 0): V | 2,
               (9 << 27, (1 << 27) + 1, 0, 0, 0, 0, 0, 0): 0, (3 << 29, 1 << 29, 0, 0, 0, 0, 0, 0): V | H | 2 | 4, (3 << 29, (1 << 29) + 1, 0, 0, 0, 0, 0, 0): V | H | 2 | 4,
               (65534, 65534, 0, 0, 65534, 65534, 0, 0): V | H | 2 | 4}
    recs = np.array(list(by_hand), np.int64).astype(np.int32)
    rc, got = _host(recs)
    assert rc == 0 and got.tolist() == list(by_hand.values()) and classify(recs).tolist() == list(by_hand.values())


@pytest.mark.parametrize("prm", [{}, dict(min_depth=1, absent_max_pm=0, het_min_pm=1, het_max_pm=999, hom_min_pm=1000),
                                 dict(min_depth=30, absent_max_pm=50, het_min_pm=300, het_max_pm=300, hom_min_pm=950)])
def test_random_records_equal_the_model(prm):
    recs = np.concatenate([random_records(20000, 5), boundary_grid(**dict(DEFAULTS, **prm))])
    rc, got = _host(recs, **prm)
    exp = classify(recs, **prm)
    assert rc == 0 and np.array_equal(got, exp)
    assert 0.05 < (exp != 0).mean() < 0.95


def test_relation_branches_and_equality():
    f = host_lib().ampli_host_concordance_relation
    cases = [(19, 19, 20, 0.8, UNDETERMINED), (0, 0, 1, 0.8, UNDETERMINED), (20, 16, 20, 0.8, SAME), (20, 15, 20, 0.8, DIFFERENT), (20, 20, 20, 1.0, SAME),
             (20, 19, 20, 1.0, DIFFERENT), (100, 80, 20, 0.8, SAME), (100, 79, 20, 0.8, DIFFERENT), (1000, 0, 20, 0.8, DIFFERENT),
             (100, 55, 1, 0.55, DIFFERENT), (100, 56, 1, 0.55, SAME), (90, 63, 1, 0.7, SAME), (90, 62, 1, 0.7, DIFFERENT), (10, 3, 1, 0.25, SAME), (40, 10, 20, 0.25, SAME), ((1 << 31) - 1, (1 << 31) - 1, 20, 1.0, SAME)]
    for he, hm, ms, sf, want in cases:
        assert f(he, hm, ms, sf) == want == relation(he, hm, ms, sf), (he, hm, ms, sf)
    # equality is decided in double as (double)het_match >= same_fraction * (double)het_either: 0.8 * 20 is 16, 0.55 * 100 rounds above 55,
    # 0.7 * 90 below 63
    assert 0.8 * 20.0 == 16.0 and 0.55 * 100.0 > 55.0 and 0.7 * 90.0 < 63.0
    rng = np.random.default_rng(3)
    for he, hm, sf in zip(rng.integers(0, 400, 3000), rng.integers(0, 400, 3000), rng.choice([0.5, 0.8, 0.9, 0.95, 1.0, 1 / 3], 3000)):
        hm = min(int(hm), int(he))
        assert f(int(he), hm, 20, float(sf)) == relation(int(he), hm, 20, float(sf))


def test_bad_parameter_sets_are_refused():
    recs = boundary_grid()[:50]
    bad = [dict(min_depth=0), dict(min_depth=-5), dict(absent_max_pm=-1), dict(absent_max_pm=250), dict(absent_max_pm=300), dict(het_min_pm=751),
           dict(het_max_pm=900), dict(het_max_pm=249), dict(hom_min_pm=1001), dict(hom_min_pm=750), dict(het_min_pm=100)]
    for prm in bad:
        rc, bits = _host(recs, **prm)
        assert rc == E_INVALID and (bits == 0xEE).all(), prm  # nothing written
    assert _host(recs, het_min_pm=750)[0] == 0 and _host(recs, hom_min_pm=1000, absent_max_pm=0)[0] == 0
