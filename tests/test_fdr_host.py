"""ampli_host_fdr_rows (libamplisolve_host.so: csrc/ampli_math.h's ampli_fdr_key / ampli_fdr_value / ampli_fdr_store with std::sort)
against the model on the grid the kernels are held to (tests/fdr_planes.py): m and rank exact, |dA| <= 1e-5, the tested mask, the sign,
+0 and NA exact, no -0 anywhere.  This pins the arithmetic of ampli_fdr_adjust without a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from amplisolve_amd import host_lib
from tests import fdr_model as fm
from tests import fdr_planes as fp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_INVALID, E_RANGE = -1, -6


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def host_fdr(s, two_sided, rank=True):
    s = np.ascontiguousarray(s, np.float32)
    rows, P = s.shape[:2]
    a, m = np.full((rows, P, 4), np.nan, np.float32), np.full((rows,), -7, np.int32)
    r = np.full((rows, P, 4), -7, np.int32) if rank else None
    assert host_lib().ampli_host_fdr_rows(_p(s), rows, P, int(two_sided), _p(a), _p(m), _p(r)) == 0
    return a, m, r


def test_the_header_states_the_constants_the_tests_use():
    hip = open(os.path.join(ROOT, "include", "amplisolve_hip.h")).read()
    math = open(os.path.join(ROOT, "amplisolve_amd", "csrc", "ampli_math.h")).read()
    types = open(os.path.join(ROOT, "include", "amplisolve_types.h")).read()
    assert int(re.search(r"#define AMPLI_FDR_TILE_KEYS (\d+)", hip).group(1)) == fp.TILE_KEYS
    assert int(re.search(r"#define AMPLI_FDR_SCAN_BLOCK (\d+)", hip).group(1)) == fp.SCAN_BLOCK
    # one definition, in the header that the other two include
    assert [m.group(1) for m in re.finditer(r"#\s*define\s+AMPLI_FDR_NA\s+(\S+)", types)] == ["(-999.0f)"]
    for t in (hip, math):
        assert not re.search(r"#\s*define\s+AMPLI_FDR_NA\b", t) and "amplisolve_types.h" in t
    assert "(C20)" in hip and "ampli_fdr_adjust" in hip and "ampli_fdr_workspace_bytes" in hip


@pytest.mark.parametrize("two_sided", [False, True])
@pytest.mark.parametrize("P", fp.edges())
def test_host_equals_the_model(P, two_sided):
    s, A, m, R = fp.case(P, two_sided)
    a, mm, r = host_fdr(s, two_sided)
    worst = fm.compare(a, mm, r, A, m, R)
    print("P", P, "two_sided", two_sided, "worst |dA|", worst, "m", m.tolist())
    k = fp.KINDS.index
    assert m[k("all_na")] == 0 and (a[k("all_na")] == np.float32(fm.NA)).all()
    assert m[k("one_tested")] == 1 and (r[k("one_tested")] == 1).sum() == 1
    if not two_sided:
        assert (a[k("one_tested")] == np.float32(17.25)).sum() == 1  # A = a
    assert (a[k("all_zero")][s[k("all_zero")][..., 0] == 0] == 0).all()
    # without the ranks: the same bytes
    a2, m2, _ = host_fdr(s, two_sided, rank=False)
    assert a2.tobytes() == a.tobytes() and m2.tobytes() == mm.tobytes()


@pytest.mark.parametrize("two_sided", [False, True])
def test_key_rules_one_by_one(two_sided):
    """every rule as its own one-cell row beside a fixed tested cell (5, 9): the class shows in m and in the stored value"""
    cells = [(-1.0, -1.0), (-1.0, 5.0), (0.0, -1.0), (-888.0, 5.0), (5.0, -888.0), (-999.0, -999.0), (-999.0, 3.0), (np.nan, 5.0), (5.0, np.nan),
             (np.inf, 5.0), (5.0, -np.inf), (100.0001, 5.0), (5.0, -100.0001), (100.0, 100.0), (-0.0, 7.0), (7.0, -0.0), (-0.0, -0.0), (3.0, 7.0),
             (3.0, -7.0), (-3.0, -7.0), (-7.0, -3.0), (-100.0, -100.0)]
    s = np.full((len(cells), 1, 4, 2), -999.0, np.float32)
    s[:, 0, 0] = (5.0, 9.0)
    s[:, 0, 2] = np.array(cells, np.float32)
    a, m, r = host_fdr(s, two_sided)
    fm.compare(a, m, r, *fm.adjust(s, two_sided))
    _, cls = fm.keys(s, two_sided)
    assert np.array_equal(m, (cls != fm.UNTESTED).sum(axis=(1, 2)))
    for i, c in enumerate(cells):
        got = a[i, 0, 2]
        if cls[i, 0, 2] == fm.UNTESTED:
            assert got == np.float32(fm.NA) and m[i] == 1, c
        elif cls[i, 0, 2] == fm.ZERO:
            assert got == 0 and not np.signbit(got) and r[i, 0, 2] == 0 and m[i] == 2, c
        else:
            assert m[i] == 2 and r[i, 0, 2] >= 1 and (got <= 0 if cls[i, 0, 2] == fm.MINUS else got >= 0), c
    # -0.0f among positives is not the largest key: the positive cell beside it keeps rank 1
    i = cells.index((-0.0, 7.0))
    assert r[i, 0, 0] == 1 and r[i, 0, 2] == 0


def test_a_score_plane_with_fitted_dispersion_values_is_just_a_plane():
    """values as ampli_nb_score_records writes them: -1 (NA), -888, 0 and clamped hundreds"""
    rng = np.random.default_rng(3)
    s = rng.choice(np.array([-1.0, -888.0, 0.0, 0.4, 2.5, 13.0, 47.0, 100.0], np.float32), (3, 300, 4, 2))
    a, m, r = host_fdr(s, False)
    fm.check(a, m, r, s, False)


def test_refusals():
    s = np.zeros((2, 3, 4, 2), np.float32)
    a, m = np.full((2, 3, 4), 7.0, np.float32), np.full((2,), 7, np.int32)
    L = host_lib()
    bad = [L.ampli_host_fdr_rows(None, 2, 3, 0, _p(a), _p(m), None), L.ampli_host_fdr_rows(_p(s), 2, 3, 0, None, _p(m), None),
           L.ampli_host_fdr_rows(_p(s), 2, 3, 0, _p(a), None, None), L.ampli_host_fdr_rows(_p(s), 0, 3, 0, _p(a), _p(m), None),
           L.ampli_host_fdr_rows(_p(s), 2, 0, 0, _p(a), _p(m), None), L.ampli_host_fdr_rows(_p(s), 2, -1, 0, _p(a), _p(m), None),
           L.ampli_host_fdr_rows(_p(s), 2, 3, 2, _p(a), _p(m), None), L.ampli_host_fdr_rows(_p(s), 2, 3, -1, _p(a), _p(m), None)]
    assert bad == [E_INVALID] * len(bad)
    assert L.ampli_host_fdr_rows(_p(s), 2, 1 << 29, 0, _p(a), _p(m), None) == E_RANGE
    assert (a == 7.0).all() and (m == 7).all()
