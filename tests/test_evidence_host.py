"""ampli_host_evidence_score, the host library's twin of ampli_evidence_score (the same ampli_ev_* of csrc/ampli_math.h compiled for the
host), against the numpy model without a device: every integer equal, z2 equal in its uint64 view."""
import ctypes as C

import numpy as np
import pytest

from tests import evidence_model as em


def host_score(planes, ref, alt):
    from amplisolve_amd import host_lib

    planes = np.ascontiguousarray(planes, np.int32)
    P = len(planes)
    ref, alt = np.ascontiguousarray(ref, np.int8), np.ascontiguousarray(alt, np.int8)
    ints, med = np.full((P, em.METRICS, 3), 7, np.int64), np.full((P, em.METRICS, 2), 7, np.int32)
    z2, used = np.full((P, em.METRICS), 7.0, np.float64), np.full(P, 7, np.int8)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert host_lib().ampli_host_evidence_score(ptr(planes), P, ptr(ref), ptr(alt), ptr(ints), ptr(med), ptr(z2), ptr(used)) == 0
    return em.Score(ints, med, z2, used)


@pytest.mark.parametrize("name", [c[0] for c in em.score_cases()])
def test_score_cases_bit_for_bit(name):
    _, planes, ref, alt = next(c for c in em.score_cases() if c[0] == name)
    found = em.score_differences(host_score(planes, ref, alt), em.score(planes, ref, alt))
    assert not found, found


def test_random_planes_bit_for_bit():
    planes, ref, alt = em.random_planes(np.random.default_rng(2902), 400)
    want = em.score(planes, ref, alt)
    assert (want.ints[:, :, 2] >= 0).sum() >= 200 and (want.z2 < 0).sum() >= 50 and (want.z2 > 0).sum() >= 50
    found = em.score_differences(host_score(planes, ref, alt), want)
    assert not found, found


def test_the_planes_of_a_counted_stream_bit_for_bit():
    case = next(c for c in em.cases() if c.name.endswith("_dense"))
    planes = case.want().hist
    rng = np.random.default_rng(2903)
    ref = rng.integers(0, 4, size=len(planes))
    for alt in (np.full(len(planes), -1), (ref + 1 + rng.integers(0, 3, size=len(planes))) % 4):
        found = em.score_differences(host_score(planes, ref, alt), em.score(planes, ref, alt))
        assert not found, found


def test_arguments():
    from amplisolve_amd import host_lib

    lib = host_lib()
    one = np.zeros((1, 4, em.METRICS, em.BINS), np.int32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    good = [ptr(one), 1, ptr(np.zeros(1, np.int8)), ptr(np.zeros(1, np.int8)), ptr(np.zeros(9, np.int64)), ptr(np.zeros(6, np.int32)), ptr(np.zeros(3)), ptr(np.zeros(1, np.int8))]
    assert lib.ampli_host_evidence_score(*good) == 0
    for at in (0, 2, 3, 4, 5, 6, 7):
        args = list(good)
        args[at] = None
        assert lib.ampli_host_evidence_score(*args) != 0, at
    assert lib.ampli_host_evidence_score(good[0], -1, *good[2:]) != 0
    assert lib.ampli_host_evidence_score(good[0], 0, *good[2:]) == 0
