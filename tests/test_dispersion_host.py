"""ampli_host_dispersion_cell_batch -- the finalize arithmetic of one cell (csrc/ampli_math.h, what dispersion_finalize_kernel runs) --
against the exact definition (tests/dispersion_model.py) on random cells and on the edges n = 0, 1, 2, K = 0, 1, 2 and equal depths."""
import ctypes as C
import math
from fractions import Fraction

import numpy as np

from amplisolve_amd import host_lib
from tests.dispersion_model import FEW, HIGH, OK, cell_exact

Z_CUTOFF = 4.0


def _batch(cells, z_cutoff=Z_CUTOFF):
    """cells: (n, K, D, x2, rinv) with x2 and rinv as doubles"""
    n = np.array([c[0] for c in cells], np.int32)
    K, D, x2, rinv = (np.array([c[i] for c in cells], np.float64) for i in (1, 2, 3, 4))
    z, phi, st = np.empty(len(cells), np.float64), np.empty(len(cells), np.float32), np.empty(len(cells), np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    host_lib().ampli_host_dispersion_cell_batch(p(n), p(K), p(D), p(x2), p(rinv), len(cells), z_cutoff, p(z), p(phi), p(st))
    return z, phi, st


def _check(ks, ds):
    cells, want = [], []
    for k, d in zip(ks, ds):
        n, K, D, X2, RI, V = cell_exact(k, d)
        few = X2 is None
        cells.append((n, K, D, 0.0 if few else float(X2), 0.0 if few else float(RI)))
        want.append(None if few else (float(X2 - (n - 1)) / math.sqrt(float(V)), float(X2 / (n - 1)), K))
    z, phi, st = _batch(cells)
    worst = 0.0
    for i, w in enumerate(want):
        if w is None:
            assert (st[i], z[i], phi[i]) == (FEW, 0.0, 0.0), (cells[i], st[i], z[i], phi[i])
            continue
        zz, ph, K = w
        worst = max(worst, abs(z[i] - zz) / (1 + K + abs(zz)))
        assert abs(z[i] - zz) <= 1e-12 * (1 + K + abs(zz)), (cells[i], z[i], zz)
        assert abs(phi[i] - ph) <= 2e-7 * abs(ph), (cells[i], phi[i], ph)
        if abs(zz - Z_CUTOFF) > 1e-9 * (1 + abs(zz)):
            assert st[i] == (HIGH if zz >= Z_CUTOFF else OK), (cells[i], st[i], zz)
        else:
            assert st[i] in (OK, HIGH)
    return worst


def test_random_cells():
    rng = np.random.default_rng(7)
    ks, ds = [], []
    for _ in range(3000):
        n = int(rng.choice([2, 3, 7, 11, 64, 256]))
        d = rng.integers(1, int(rng.choice([50, 3000, 250_000])) + 1, n)
        lam = rng.choice([0.0005, 0.003, 0.03]) * d * (rng.gamma(0.5, 2.0, n) if rng.random() < 0.4 else 1.0)
        ks.append([int(v) for v in np.minimum(rng.poisson(lam), d)])
        ds.append([int(v) for v in d])
    worst = _check(ks, ds)
    print(f"z against the exact definition: worst {worst:.3g} of (1 + K + |z|)")


def test_edges():
    ks = [[], [5], [0, 0], [1, 0], [0, 1], [1, 1], [2, 0], [0, 2], [3, 4], [0, 0, 0], [1, 0, 0], [0, 1, 1], [2, 2, 2, 2], [7, 0, 0, 0, 0, 0, 0],
          [1] * 64, [0] * 63 + [2], [40, 1, 1, 1]]
    ds = [[100 + 37 * i for i in range(len(k))] for k in ks]
    _check(ks, ds)
    _check(ks, [[2000] * len(k) for k in ks])  # all d equal: D sum 1/d = n^2, V = 2 (n - 1)(1 - 1/K)
    n, K = 9, 13
    z, phi, st = _batch([(n, K, n * 2000, 8.0, n / 2000)])
    assert abs(z[0] - 0.0) < 1e-12 and st[0] == OK and abs(phi[0] - 1.0) < 1e-7
    V = float(2 * (n - 1) - Fraction(2 * n - 2, K))
    z, _, st = _batch([(n, K, n * 2000, 8.0 + 5.0 * math.sqrt(V), n / 2000)])
    assert abs(z[0] - 5.0) < 1e-12 and st[0] == HIGH


def test_cutoff_is_inclusive_and_signed():
    cell = (7, 40.0, 14000.0, 6.0, 7 / 2000)  # X2 = n - 1: z = 0 exactly
    assert _batch([cell], 0.0)[2][0] == HIGH
    assert _batch([cell], 1e-300)[2][0] == OK
    assert _batch([cell], -3.0)[2][0] == HIGH
