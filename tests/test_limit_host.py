"""Detection limits without a GPU: the exports, the host's literal scan against the model, the kernel's search (ampli_math.h, through
the host library) against both, and the three properties of the scorer the search rests on, on the CPU oracle."""
import ctypes as C

import numpy as np

from amplisolve_amd import _lib, host_lib
from oracle import pyoracle as orc
from tests.helpers import borderline_triples
from tests.limit_model import strand_limit


def _search(depth, thr, bound):
    ev = C.c_int32(0)
    return host_lib().ampli_host_limit_search(int(depth), float(thr), int(bound), C.byref(ev)), ev.value


def test_exports_and_abi_version():
    lib = C.CDLL(_lib.HIP_LIB_PATH)
    assert hasattr(lib, "ampli_limit_records") and hasattr(lib, "ampli_limit_stats")
    assert hasattr(C.CDLL(_lib.HOST_LIB_PATH), "ampli_host_limit_reads")
    assert _lib.hip_lib().ampli_abi_version() == 5


def test_host_scan_and_search_equal_the_model_on_a_grid():
    H = host_lib()
    n = 0
    for depth in (-7, 0, 1, 20, 100, 999, 1000, 2000, 63000):
        # 0.003 * 1000 = 3.00000003, 0.007 * 1000 = 6.9999999, 0.002 * 1000 = 2.00000009: m next to an integer on either side
        for thr in (-1.0, 0.0, 0.0001, 0.001, 0.002, 0.003, 0.007, 0.01, 0.05, 0.9):
            m = max(0.0, depth * float(np.float32(thr if thr else 0.0010008)))
            for bound in sorted({1, 2, 3, max(1, int(m)), int(m) + 1, int(m) + 2, int(m + 2 * (m + 1) ** 0.5) + 3, max(1, depth)}):
                want = strand_limit(depth, thr, bound)
                assert H.ampli_host_limit_reads(depth, thr, bound) == want, (depth, thr, bound)
                got, ev = _search(depth, thr, bound)
                assert got == want, (depth, thr, bound, got, want)  # no RECHECK: every mean of the grid is positive and finite, no Q in the band
                assert ev <= 128
                n += want == 0
    assert n > 20  # bounds below the limit: UNREACHABLE
    # means the search does not take: negative, NaN, infinite -> RECHECK (-2), and the literal scan says what the reference would
    for depth, thr in ((1000, -0.5), (1000, float("nan")), (1000, float("inf"))):
        assert _search(depth, thr, 50)[0] == -2
        assert H.ampli_host_limit_reads(depth, thr, 50) == strand_limit(depth, thr, 50)


def test_borderline_counts_are_rechecked_not_guessed():
    H = host_lib()
    trip = borderline_triples(want=12)
    assert len(trip) >= 6
    n_recheck = 0
    for k, rd, err, q in trip:
        for bound in (k - 1, k, k + 3):
            want = strand_limit(rd, err, bound, from_one=False)
            assert H.ampli_host_limit_reads(rd, err, bound) == want, (k, rd, err, bound)
            got, _ = _search(rd, err, bound)
            assert got in (-2, want), (k, rd, err, q, bound, got, want)
            n_recheck += got == -2
    assert n_recheck > 0  # Q(k) lies within 1e-6 of the gate in every triple: the walk that reaches k must stop there


def test_properties_the_search_rests_on():
    """on 120 000 random strands (depth 20 .. 63 000 log-uniform, thresholds 1e-4 .. 0.05 rounded as the table's %f text):
    (1) nothing passes at k <= m; (2) every count above the first passing one passes; (3) the first passing count is not below the
    seed (floor(m + 0.4 sqrt(m + 1)) for m <= 1024, floor(m) + 1 beyond) and at most 100 steps above it (AMPLI_LIMIT_MAX_EVALS is 128); and the kernel's search lands on it."""
    rng = np.random.default_rng(20261016)
    N = 120_000
    depth = np.exp(rng.uniform(np.log(20), np.log(63000), N)).astype(np.int32)
    thr = np.array([float(f"{x:f}") for x in np.exp(rng.uniform(np.log(1e-4), np.log(0.05), N))], np.float32)
    m = depth.astype(np.float64) * thr.astype(np.float64)
    fl = np.floor(m).astype(np.int32)
    has = fl >= 1
    q, _ = orc.score_batch(fl[has], depth[has], thr[has])
    assert (q < 5).all()                                       # (1) at k = floor(m), the largest k <= m
    k_lo = np.maximum(1, (fl[has] * rng.random(has.sum())).astype(np.int32))
    q, _ = orc.score_batch(k_lo, depth[has], thr[has])
    assert (q < 5).all()                                       # (1) at a random k <= m
    first = np.zeros(N, np.int32)
    k = fl + 1
    todo = np.arange(N)
    steps = 0
    while todo.size:
        q, _ = orc.score_batch(k[todo], depth[todo], thr[todo])
        done = q >= 5
        first[todo[done]] = k[todo[done]]
        todo = todo[~done]
        k[todo] += 1
        steps += 1
        assert steps < 200
    for above in (1, 2, 3, 7, 50, 1000):                        # (2)
        q, _ = orc.score_batch(first + above, depth, thr)
        assert (q >= 5).all()
    q, _ = orc.score_batch(first + (rng.random(N) * 3 * np.sqrt(m + 1)).astype(np.int32), depth, thr)
    assert (q >= 5).all()
    seed = np.where(m <= 1024, np.maximum(fl + 1, np.floor(m + 0.4 * np.sqrt(m + 1)).astype(np.int32)), fl + 1)  # ampli_limit_init
    assert (first >= seed).all()                               # (3)
    assert (first - seed).max() < 100
    q_at, _ = orc.score_batch(first, depth, thr)
    q_below, _ = orc.score_batch(first - 1, depth, thr)
    in_band = (np.abs(q_at - 5) <= 1e-6) | ((first - 1 > m) & (np.abs(q_below - 5) <= 1e-6))
    n_recheck = 0
    evals = []
    for i in range(0, N, 4):                                   # the search itself on 30 000 of them
        got, ev = _search(depth[i], thr[i], 1 << 30)
        n_recheck += got == -2
        assert got == first[i] or (got == -2 and in_band[i]), (depth[i], thr[i], got, first[i])
        evals.append(ev)
    assert n_recheck <= 0.01 * (N // 4)
    assert max(evals) <= 128 and np.mean(evals) < 6


def test_search_at_depths_beyond_the_table():
    """depths up to 2^30 (the int32 layout): the series is cut at its 99th term long before it converges, the first passing count falls
    back towards floor(m) + 1, and the search -- unseeded there, kf_lgamma by the Lanczos form -- still lands on the model's count"""
    rng = np.random.default_rng(7)
    worst = 0
    for _ in range(1500):
        depth = int(np.exp(rng.uniform(np.log(20000), np.log(2 ** 30))))
        thr = float(np.float32(float(f"{np.exp(rng.uniform(np.log(1e-4), np.log(0.05))):f}")))
        got, ev = _search(depth, thr, depth)
        assert got == strand_limit(depth, thr, depth, from_one=False), (depth, thr)
        worst = max(worst, ev)
    assert worst <= 64
