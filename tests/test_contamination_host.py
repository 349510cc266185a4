"""ampli_host_contamination_estimate (csrc/ampli_math.h's ampli_contamination_estimate: the text the command line runs, compiled for the
host) against the definition in tests/contamination_model.py, bit for bit: 20 000 random sum vectors -- small, large, with and without a
background, with and without het depth -- and every branch: den == 0, s8 == 0, num < 0, the status at its bounds."""
import ctypes as C
import math
import struct

import numpy as np

from amplisolve_amd import host_lib
from tests.contamination_model import CLEAN, CONTAMINATED, UNDETERMINED, estimate, status

E_INVALID = -1


def _host(s, min_sites=20, min_fraction=0.005):
    v = np.ascontiguousarray(s, np.int64)
    f, se, e = C.c_double(7.0), C.c_double(7.0), C.c_double(7.0)
    rc = host_lib().ampli_host_contamination_estimate(v.ctypes.data_as(C.c_void_p), min_sites, min_fraction, C.byref(f), C.byref(se), C.byref(e))
    return rc, f.value, se.value, e.value


def _bits(x):
    return struct.pack("<d", x) if x == x else b"nan"  # every NaN is one NaN


def _same(s, min_sites=20, min_fraction=0.005):
    rc, f, se, e = _host(s, min_sites, min_fraction)
    mf, mse, me = estimate(s)
    assert rc == status(s, min_sites, min_fraction), s
    assert (_bits(f), _bits(se), _bits(e)) == (_bits(mf), _bits(mse), _bits(me)), (s, f, mf, se, mse, e, me)
    return rc, f, se, e


def test_branches():
    rc, f, se, e = _same([0] * 9)
    assert rc == UNDETERMINED and math.isnan(f) and math.isnan(se) and e == 0.0                 # den == 0
    rc, f, se, e = _same([25, 0, 0, 0, 0, 0, 0, 0, 0])
    assert rc == CLEAN and math.isnan(f)                                                         # sites without depth: never contaminated
    rc, f, se, e = _same([10, 50, 5000, 10, 0, 0, 0, 0, 0])
    assert rc == CONTAMINATED and f == 0.01 and e == 0.0                                         # s8 == 0
    rc, f, se, e = _same([20, 2, 5000, 0, 0, 0, 100, 900, 100000])
    assert rc == CLEAN and f == 0.0 and math.copysign(1.0, f) == 1.0 and e == 0.003              # num < 0 clamps to +0
    rc, f, se, e = _same([10, 50, 5000, 10, 30, 4000, 100, 300, 100000])
    assert rc == CONTAMINATED and f == (80.0 - 0.001 * 9000.0) / 7000.0
    assert _same([10, 50, 5000, 9, 30, 4000, 100, 300, 100000])[0] == UNDETERMINED               # 19 sites
    s = [20, 50, 10000, 0, 0, 0, 0, 0, 0]
    assert _same(s, 20, 0.005)[0] == CONTAMINATED and _same(s, 20, 0.0050000001)[0] == CLEAN      # equality is contaminated
    big = [1 << 20, 1 << 50, 1 << 58, 1 << 20, 1 << 49, 1 << 58, 1 << 30, 1 << 48, 1 << 58]
    assert _same(big)[0] == CLEAN
    assert host_lib().ampli_host_contamination_estimate(None, 20, 0.005, None, None, None) == E_INVALID
    v = np.array([20, 50, 10000, 0, 0, 0, 0, 0, 0], np.int64)
    assert host_lib().ampli_host_contamination_estimate(v.ctypes.data_as(C.c_void_p), 20, 0.005, None, None, None) == CONTAMINATED


def test_random_sum_vectors_equal_the_model_bit_for_bit():
    rng = np.random.default_rng(15)
    n = 20000
    scale = rng.choice([1, 10, 1000, 10 ** 5, 10 ** 7, 10 ** 10, 1 << 40], size=(n, 1))
    depth = (rng.random((n, 3)) * scale * 1000).astype(np.int64)          # depth_hom, depth_het, depth_bg
    share = rng.choice([0.0, 1e-4, 7e-4, 0.003, 0.01, 0.08, 0.3], size=(n, 3))
    alt = (depth * share * rng.random((n, 3))).astype(np.int64)
    sites = rng.integers(0, 40, (n, 3))
    S = np.stack([sites[:, 0], alt[:, 0], depth[:, 0], sites[:, 1], alt[:, 1], depth[:, 1], sites[:, 2], alt[:, 2], depth[:, 2]], axis=1)
    S[rng.random(n) < 0.1, 5] = 0   # no het depth
    S[rng.random(n) < 0.1, 2] = 0   # no hom depth
    S[rng.random(n) < 0.1, 8] = 0   # no background
    seen = set()
    nan = clamped = 0
    for s in S:
        rc, f, se, e = _same(s.tolist())
        seen.add(rc)
        nan += f != f
        clamped += f == 0.0
    assert seen == {UNDETERMINED, CLEAN, CONTAMINATED} and nan > 50 and clamped > 50
