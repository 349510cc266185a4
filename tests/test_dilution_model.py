"""The model of the in-silico dilution (tests/dilution_model.py) on its own: the generator's known answers, the identities of
Thin, and the generator as a sampler.  The sampler's bounds are conditions on a correct Philox with this counter layout, not
measurements: the figures this definition gives (z 0.09, -1.31, 0.75, -0.81; dispersion 0.973, 1.032, 0.991, 0.966; r -0.027, 0.013,
-0.009) are asserted to three decimals beside them, so that a counter layout that differs from the text cannot pass."""
import functools

import numpy as np
import pytest

from tests import dilution_model as dm

KEY = 0x0123456789ABCDEF


def test_known_answers():
    for ctr, key, want in dm.KNOWN:
        assert tuple(int(x) for x in dm.philox(*ctr, *key)) == want


def test_keep_of_fractions():
    assert dm.keep_of(0.0) == 0 and dm.keep_of(1.0) == 1 << 32 and dm.keep_of(0.5) == 1 << 31
    assert dm.keep_of(0.1) == 429496730 and dm.keep_of(2.0 ** -33) == 1 and dm.keep_of(2.0 ** -34) == 0  # floor(x + 0.5): a half goes up


def test_identities_hold_exactly():
    rng = np.random.default_rng(3)
    n = rng.integers(0, 3000, 200)
    keep = rng.integers(0, (1 << 32) + 1, 200).astype(np.uint64)
    keep[:4] = [0, 1, (1 << 32) - 1, 1 << 32]
    p, fs = rng.integers(0, 1 << 31, 200), rng.integers(0, 16, 200)
    base = dm.thin_cells(n, keep, KEY, p, fs)
    assert (base >= 0).all() and (base <= n).all()
    assert (dm.thin_cells(n + rng.integers(0, 9, 200), keep, KEY, p, fs) >= base).all()                           # monotone in n
    more = np.minimum(keep + rng.integers(0, 1 << 28, 200).astype(np.uint64), np.uint64(1 << 32))
    assert (dm.thin_cells(n, more, KEY, p, fs) >= base).all()                                                     # monotone in keep
    assert np.array_equal(dm.thin_cells(n, 1 << 32, KEY, p, fs), n) and not dm.thin_cells(n, 0, KEY, p, fs).any()  # all, none
    assert dm.thin(0, 1 << 31, KEY, 0, 0, 0) == 0


@functools.lru_cache(maxsize=None)
def _sample(frac, n):
    # floor, not keep_of's floor(x + 0.5): the recorded figures below were taken with keep = floor(fraction * 2^32), as the correlation case states
    keep = int(np.floor(np.ldexp(frac, 32)))
    got = dm.thin_cells(np.full(2000, n), keep, KEY, np.repeat(np.arange(250), 8), np.tile(np.arange(8), 250))
    return got, keep / 2.0 ** 32


@pytest.mark.parametrize("frac,n,z_is,disp_is", [(0.1, 1000, 0.09, 0.973), (0.01, 6000, -1.31, 1.032), (0.5, 257, 0.75, 0.991), (0.001, 20000, -0.81, 0.966)])
def test_generator_as_a_sampler(frac, n, z_is, disp_is):
    got, q = _sample(frac, n)
    z = (got.sum() - 2000 * n * q) / np.sqrt(2000 * n * q * (1 - q))
    disp = float(np.mean((got - n * q) ** 2 / (n * q * (1 - q))))
    print(f"fraction {frac} n {n}: z {z:.3f} dispersion {disp:.4f}")
    assert abs(z) <= 4.0 and 0.9 <= disp <= 1.1
    assert round(float(z), 2) == z_is and round(disp, 3) == disp_is


def test_sides_fields_and_keys_are_uncorrelated():
    keep, p, n = int(np.floor(0.1 * 2.0 ** 32)), np.arange(2000), np.full(2000, 1000)
    base = dm.thin_cells(n, keep, KEY, p, 0)
    r = [float(np.corrcoef(base, x)[0, 1]) for x in (dm.thin_cells(n, keep, KEY, p, 8), dm.thin_cells(n, keep, KEY, p, 1), dm.thin_cells(n, keep, KEY + 1, p, 0))]
    print("r between the sides, fields 0 and 1, key and key + 1:", [f"{x:.4f}" for x in r])
    assert all(abs(x) <= 0.1 for x in r)
    assert [round(x, 3) for x in r] == [-0.027, 0.013, -0.009]


def test_mixture_rules_on_a_tiny_chunk():
    """absent records, a named b, down-sampling, a bad count and a bad mixture, cell by cell through thin()"""
    A = np.array([[[10, 2, 0, 0, 9, 1, 0, 0], [dm.ABSENT, 0, 0, 0, 0, 0, 0, 0], [5, 0, 0, 1 << 24, 5, 0, 0, 0]]], np.int32)
    B = np.array([[[100, 0, 3, 0, 90, 0, 2, 0], [7, 0, 0, 0, 7, 0, 0, 0], [1, 1, 1, 1, 1, 1, 1, 1]]], np.int32)
    ka, kb = dm.keep_of(0.5), dm.keep_of(0.25)
    out, flags = dm.dilute_model(A, B, 3, [(0, 0, ka, kb, KEY), (0, -1, ka, kb, KEY), (1, 0, ka, kb, KEY), (0, -1, (1 << 32) + 1, 0, KEY)])
    assert list(flags) == [dm.BAD_COUNT, dm.BAD_COUNT, dm.BAD_MIXTURE, dm.BAD_MIXTURE]
    want0 = [dm.thin(int(A[0, 0, f]), ka, KEY, 0, f, 0) + dm.thin(int(B[0, 0, f]), kb, KEY, 0, f, 1) for f in range(8)]
    assert list(out[0, 0]) == want0 and list(out[1, 0]) == [dm.thin(int(A[0, 0, f]), ka, KEY, 0, f, 0) for f in range(8)]
    absent = [dm.ABSENT, 0, 0, 0, 0, 0, 0, 0]
    assert all(list(out[m, p]) == absent for m, p in ((0, 1), (0, 2), (1, 1), (1, 2))) and (out[2:, :, 0] == dm.ABSENT).all() and not out[2:, :, 1:].any()
    # nested: with one key the reads kept at the smaller fraction are among those kept at the larger -- count by count
    small, _ = dm.dilute_model(B, None, 3, [(0, -1, dm.keep_of(0.1), 0, KEY)])
    large, _ = dm.dilute_model(B, None, 3, [(0, -1, dm.keep_of(0.4), 0, KEY)])
    assert (small <= large).all() and (small < large).any()
