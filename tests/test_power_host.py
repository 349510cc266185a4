"""Detection power without a GPU: the pure-Python definition (tests/power_model.py) pinned to scipy and mpmath, and the code
the kernel runs (csrc/ampli_math.h through the host library: ampli_host_binom_tail, ampli_host_power_pair) against that definition --
tails within 1e-6 absolute, the LoD within 1e-4 relative, tails monotone in v and in k, the terms of a tail inside the stated bound."""
import ctypes as C
import math

import numpy as np
import pytest

from amplisolve_amd import _lib, host_lib
from tests import power_model as pm
from tests.test_gpu_limits import LEVELS

TAIL_TOL = 1e-6   # the project's tolerance on a probability
LOD_TOL = 1e-4    # relative; DESIGN 12: d power / d ln v >= 0.046 at the root for c <= 0.99, so 1e-6 of power is <= 2.2e-5 of ln v
DEPTHS = (1, 2, 100, 5183, 65534, 262136, 1 << 24, 1 << 30)
CONFIDENCES = (0.5, 0.95, 0.99)


def _tail(n, k, v):
    t = C.c_int32(-1)
    return host_lib().ampli_host_binom_tail(int(n), int(k), float(v), C.byref(t)), t.value


def _pair(FW, kf, BW, kb, levels, c, want_lod=True):
    lv = (C.c_float * max(1, len(levels)))(*levels)
    pw = (C.c_double * max(1, len(levels)))()
    lod, it = C.c_double(0), C.c_int32(0)
    rc = host_lib().ampli_host_power_pair(FW, kf, BW, kb, lv, len(levels), c, pw, C.byref(lod) if want_lod else None, C.byref(it))
    return rc, list(pw)[:len(levels)], lod.value, it.value


def _grid():
    out = []
    for n in DEPTHS:
        for lv in LEVELS:
            v = float(np.float32(lv))
            m = n * v
            for k in sorted({1, 2, round(m), round(m) + 1, round(m) - 1, round(m) + round(3 * math.sqrt(m)), round(m) - round(3 * math.sqrt(m)), n}):
                if 1 <= k <= n:
                    out.append((n, k, v))
    return out


def _random_triples(N, seed):
    """n log-uniform in 1 .. 2^30, the mean n v log-uniform in 0.01 .. min(n, 1e5), k within four standard deviations of it (the deep
    means are the grid's: a pure-Python sum of 100 000 terms per triple would take minutes)"""
    rng = np.random.default_rng(seed)
    n = np.exp(rng.uniform(0, np.log(2.0 ** 30), N)).astype(np.int64)
    m = np.exp(rng.uniform(np.log(0.01), np.log(np.minimum(n, 1e5))))
    v = np.minimum(m / n, 0.999)
    k = np.rint(n * v + rng.uniform(-4, 4, N) * np.sqrt(n * v * (1 - v))).astype(np.int64)
    return list(zip(n.tolist(), np.clip(k, 1, n).tolist(), v.tolist()))


def test_exports_and_abi_version():
    lib = C.CDLL(_lib.HIP_LIB_PATH)
    assert hasattr(lib, "ampli_power_records") and hasattr(lib, "ampli_power_stats")
    host = C.CDLL(_lib.HOST_LIB_PATH)
    assert hasattr(host, "ampli_host_binom_tail") and hasattr(host, "ampli_host_power_pair")
    assert _lib.hip_lib().ampli_abi_version() == 5


def test_model_is_pinned_to_scipy_and_mpmath():
    sp = pytest.importorskip("scipy.special")
    mpmath = pytest.importorskip("mpmath")
    grid = [g for g in _grid() if g[2] < 1]
    # scipy's betainc is itself only good to ~1e-8 at 2^30 (it differs from the 40-digit sum by that much there): 1e-7
    assert max(abs(pm.tail(n, k, v) - float(sp.betainc(k, n - k + 1, v))) for n, k, v in grid) <= 1e-7

    def mp_tail(n, k, v):
        """the same sum at 40 digits, every term's start from mpmath.loggamma"""
        v = mpmath.mpf(v)
        q = 1 - v
        up = k > n * v
        j = k if up else k - 1
        t = mpmath.exp(mpmath.loggamma(n + 1) - mpmath.loggamma(j + 1) - mpmath.loggamma(n - j + 1) + j * mpmath.log(v) + (n - j) * mpmath.log(q))
        s, floor = t, t * mpmath.mpf("1e-45")
        while (j < n) if up else (j > 0):
            t *= (mpmath.mpf(n - j) / (j + 1) * v / q) if up else (mpmath.mpf(j) / (n - j + 1) * q / v)
            j += 1 if up else -1
            if t < floor:
                break
            s += t
        return float(s if up else 1 - s)

    with mpmath.workdps(40):
        few = [g for g in grid if g[0] * g[2] * (1 - g[2]) <= 3e4] + [(1 << 30, round((1 << 30) * 0.001) + 300, float(np.float32(0.001)))]
        worst = max(abs(pm.tail(n, k, v) - mp_tail(n, k, v)) for n, k, v in few)
    print(f"model against the 40-digit sum on {len(few)} triples: {worst:.3g}")
    assert len(few) > 200 and worst <= 1e-11  # fp64 rounding of a few thousand terms; six orders inside TAIL_TOL


def test_host_tail_equals_the_model_and_its_terms_are_bounded():
    worst = most = 0.0
    n_sum = n_cut = 0
    for n, k, v in _grid() + _random_triples(20_000, 20261018):
        got, terms = _tail(n, k, v)
        err = abs(got - pm.tail(n, k, v))
        worst = max(worst, err)
        assert err <= TAIL_TOL, (n, k, v, got)
        # the bound of csrc/ampli_math.h (AMPLI_TAIL_TERMS): 8 standard deviations and 64 terms
        assert 0 <= terms <= 8 * math.sqrt(n * v * (1 - v)) + 64, (n, k, v, terms)
        most = max(most, terms / (8 * math.sqrt(n * v * (1 - v)) + 64))
        n_sum += terms > 1
        n_cut += terms == 1 and 0 < v < 1 and got in (0.0, 1.0)
    print(f"host tail against the model: worst {worst:.3g}; most terms / bound {most:.3f}; {n_sum} summed, {n_cut} decided by the Chernoff bound")
    assert n_sum > 5000 and n_cut > 50
    # far from the mean at depth: decided, not summed
    for n, k, v in ((1 << 30, 1, 0.1), (1 << 30, (1 << 30) // 20, 0.1), (1 << 30, (1 << 30) // 5, 0.1), (1 << 30, 1 << 30, 0.1)):
        got, terms = _tail(n, k, v)
        assert terms <= 1 and got == (1.0 if k < n * v else 0.0)
    assert _tail(100, 0, 0.5) == (1.0, 0) and _tail(100, 101, 0.5) == (0.0, 0) and _tail(100, 3, 1.0) == (1.0, 0) and _tail(100, 3, 0.0) == (0.0, 0)


def test_tails_are_monotone_in_v_and_in_k():
    """up to 1e-10: a sum is cut once what is left is below 1e-11, and its first term carries ~1e-16 |k - n v| of relative error"""
    slack = 1e-10
    for n in (1, 2, 100, 5183, 65534, 1 << 24, 1 << 30):
        for v in (0.001, 0.01, 0.1, 0.5):
            m, sd = n * v, math.sqrt(n * v * (1 - v))
            ks = sorted({min(n, max(1, round(m + z * sd))) for z in np.linspace(-7.5, 7.5, 61)} | {1, n})
            tails = [_tail(n, k, v)[0] for k in ks]
            assert all(0.0 <= t <= 1.0 for t in tails)
            assert all(b <= a + slack for a, b in zip(tails, tails[1:])), (n, v)
            k = max(1, round(m))
            vs = [v * f for f in np.exp(np.linspace(-8 / max(1.0, math.sqrt(m)), 8 / max(1.0, math.sqrt(m)), 61)) if v * f < 1]
            tails = [_tail(n, k, x)[0] for x in vs]
            assert all(a <= b + slack for a, b in zip(tails, tails[1:])), (n, v)
            assert tails[0] < 0.01 or m < 4
            assert tails[-1] > 0.99 or m < 4 or len(vs) < 61


def _pairs(N, seed, top=1 << 30):
    """(FW, k_fw, BW, k_bw): depths log-uniform, the minimum reads around a common allele fraction or unrelated"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(N):
        FW, BW = (int(np.exp(rng.uniform(0, np.log(top)))) for _ in range(2))
        v = float(np.exp(rng.uniform(np.log(1e-4), 0)))
        ks = []
        for n in (FW, BW):
            mean = n * v if rng.random() < 0.7 else n * float(np.exp(rng.uniform(np.log(1e-4), 0)))
            ks.append(int(np.clip(round(min(mean, 3e4) + rng.uniform(-2, 2) * math.sqrt(min(mean, 3e4))), 1, n)))
        out.append((FW, ks[0], BW, ks[1]))
    return out


def test_host_lod_equals_the_model():
    worst, most = 0.0, 0
    edge = [(1, 1, 1, 1), (20, 1, 20, 1), (20, 20, 20, 20), (2000, 3, 2000, 3), (2000, 1, 100, 100), (65534, 66, 65534, 655), (1 << 24, 17000, 1 << 24, 16000),
            (1 << 30, 1, 1 << 30, 1), (1 << 30, 1 << 30, 1 << 30, 1 << 30), (1 << 30, 10_000, 1 << 28, 3000)]
    for FW, kf, BW, kb in edge + _pairs(300, 11):
        for c in CONFIDENCES:
            c32 = float(np.float32(c))
            rc, pw, lod, iters = _pair(FW, kf, BW, kb, LEVELS[:3], c)
            assert rc == 0 and 1 <= iters <= 96
            want = pm.lod(FW, kf, BW, kb, c32)
            worst = max(worst, abs(lod / want - 1))
            most = max(most, iters)
            assert abs(lod / want - 1) <= LOD_TOL, (FW, kf, BW, kb, c, lod, want)
            for got, exp in zip(pw, pm.powers(FW, kf, BW, kb, LEVELS[:3])):
                assert abs(got - exp) <= TAIL_TOL
    print(f"host LoD against the model: worst relative difference {worst:.3g}, most evaluations of a search {most}")


def test_the_slope_the_lod_tolerance_rests_on():
    """d power / d ln v at the root is at least -(1 - c) ln(1 - c), the slope of one strand that needs one read (the other tail being
    one): 0.0461 at c = 0.99, so an error of 1e-6 in the power moves ln v by at most 2.2e-5"""
    rng = np.random.default_rng(5)
    low = {c: 1e9 for c in CONFIDENCES}
    for FW, kf, BW, kb in _pairs(2000, 12, top=1 << 22):
        c = CONFIDENCES[int(rng.integers(3))]
        v = pm.lod(FW, kf, BW, kb, c)
        s = pm.slope(FW, kf, BW, kb, v)
        low[c] = min(low[c], s)
        assert s >= -(1 - c) * math.log(1 - c) * (1 - 1e-6), (FW, kf, BW, kb, c, s)
    print("smallest slope at the root:", {c: round(s, 5) for c, s in low.items()})
    assert -(1 - 0.99) * math.log(1 - 0.99) >= 0.046


def test_power_pair_refuses_what_is_not_a_pair():
    for FW, kf, BW, kb, n_levels, c in ((100, 0, 100, 1, 1, 0.95), (100, 1, 100, 101, 1, 0.95), (100, 1, 100, 1, 9, 0.95), (100, 1, 100, 1, -1, 0.95),
                                        (100, 1, 100, 1, 1, 0.4), (100, 1, 100, 1, 1, 0.995), (100, 1, 100, 1, 1, float("nan"))):
        lv = (C.c_float * 9)(*([0.01] * 9))
        pw = (C.c_double * 9)()
        assert host_lib().ampli_host_power_pair(FW, kf, BW, kb, lv, n_levels, c, pw, None, None) == -1
        assert b"power_pair" in host_lib().ampli_host_last_error()
    rc, pw, _, iters = _pair(100, 1, 100, 1, (1.0,), 0.5, want_lod=False)
    assert rc == 0 and pw == [1.0] and iters == 0
