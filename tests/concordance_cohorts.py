"""Records for the sample-identity tests (tests/test_concordance_*.py, tests/test_gpu_concordance*.py) -- TEST INFRASTRUCTURE: the
boundary grid of the genotype definition, random records around its bounds, and a planted cohort of samples drawn from a few synthetic
individuals.  Everything is computed once and shared read-only."""
import functools

import numpy as np

from tests.concordance_model import ABSENT, DEFAULTS, classify, pair_counts


def _rec(n, split=0.5):
    """a record with n[b] reads of base b, `split` of them on the forward strand"""
    n = [int(x) for x in n]
    fw = [int(x * split) for x in n]
    return fw + [x - f for x, f in zip(n, fw)]


@functools.lru_cache(maxsize=None)
def boundary_grid(min_depth=100, absent_max_pm=100, het_min_pm=250, het_max_pm=750, hom_min_pm=900):
    """int32 [k, 8]: every bound of the definition at equality and one read either side of it, at depths where pm * d is and is not a
    multiple of 1000; the depth gate; three and four het bases; counts at the 16-bit layout's maximum; 2^30 per field"""
    out = []
    for pm in (absent_max_pm, het_min_pm, het_max_pm, hom_min_pm):
        for d in (1000, 2000, 3000, 300, 1001, 777, min_depth):
            for delta in (-1, 0, 1):
                n = min(max(pm * d // 1000 + delta, 0), d)
                for split in (0.5, 0.0, 1.0, 0.3):
                    out.append(_rec([n, d - n, 0, 0], split))              # the rest in one base
                    out.append(_rec([0, (d - n) // 2, n, d - n - (d - n) // 2], split))  # the rest in two
    out += [_rec([min_depth - 1, 0, 0, 0]), _rec([min_depth, 0, 0, 0]), _rec([0, 0, min_depth - 1, 0], 0.0), _rec([0, 0, 0, min_depth], 1.0)]
    out += [_rec([250, 250, 500, 0]), _rec([250, 250, 250, 250]), _rec([500, 250, 250, 0]), _rec([1000, 1000, 1000, 1000], 0.25)]
    out += [_rec([900, 100, 0, 0]), _rec([100, 0, 0, 900], 0.1), _rec([900, 50, 50, 0]), _rec([900, 100, 100, 0])]  # HOM, a second base at absent_max
    out += [[0] * 8, [ABSENT, 0, 0, 0, 0, 0, 0, 0], [ABSENT, 500, 0, 0, 500, 0, 0, 0], [ABSENT] + [7] * 7]
    out += [[65534, 0, 0, 0, 65534, 0, 0, 0], [65534, 65534, 0, 0, 65534, 65534, 0, 0], [65534] * 8, [0, 65534, 0, 7281, 0, 65534, 0, 7282],
            [0, 65534, 0, 7282, 0, 65534, 0, 7282], [65534, 0, 21844, 0, 65534, 0, 21845, 0], [0, 0, 65534, 21845, 0, 0, 65534, 21845]]
    big = 1 << 30
    x = 1 << 27
    out += [[big] * 8, [big, 0, 0, 0, big, 0, 0, 0], [big, big, 0, 0, big, big, 0, 0], [0, big, 0, big - 1, 0, big, 0, big],
            [9 * x, x, 0, 0, 0, 0, 0, 0], [9 * x, x + 1, 0, 0, 0, 0, 0, 0], [9 * x - 1, x, 0, 0, 0, 0, 0, 0], [big, 0, big // 3, 0, big, 0, big // 3, 0],
            [(1 << 31) - 1, 0, 0, 0, (1 << 31) - 1, 0, 0, 0], [(1 << 31) - 1] * 8, [3 << 29, 1 << 29, 0, 0, 0, 0, 0, 0], [3 << 29, (1 << 29) + 1, 0, 0, 0, 0, 0, 0]]
    return np.array(out, np.int64).astype(np.int32)


def random_records(k, seed, max_count=None):
    """int32 [k, 8]: depths from a few reads to 2^22 and beyond, base fractions drawn around the four bounds, absent records"""
    rng = np.random.default_rng(seed)
    d = rng.choice([0, 1, 30, 99, 100, 101, 300, 1000, 2000, 33395, 100000, 1 << 22, 1 << 26], size=k)
    if max_count:
        d = np.minimum(d, max_count)
    frac = rng.choice([0.0, 0.001, 0.05, 0.099, 0.1, 0.101, 0.2, 0.249, 0.25, 0.251, 0.4, 0.5], size=(k, 2))
    second = rng.integers(0, 2, k).astype(bool)
    n = np.zeros((k, 4), np.int64)
    order = np.argsort(rng.random((k, 4)), axis=1)
    a1 = (d * frac[:, 0]).astype(np.int64) + rng.integers(-1, 2, k)
    a2 = np.where(second, (d * frac[:, 1]).astype(np.int64) + rng.integers(-1, 2, k), 0)
    a1, a2 = np.clip(a1, 0, d), np.clip(a2, 0, d)
    a2 = np.minimum(a2, d - a1)
    rows = np.arange(k)
    n[rows, order[:, 0]] = d - a1 - a2
    n[rows, order[:, 1]] = a1
    n[rows, order[:, 2]] = a2
    fw = rng.binomial(n, 0.5)
    recs = np.concatenate([fw, n - fw], axis=1)
    if max_count:
        recs = np.minimum(recs, max_count)
    gone = rng.random(k) < 0.05
    recs[gone, 0] = ABSENT
    return recs.astype(np.int32)


@functools.lru_cache(maxsize=None)
def records(P, n, seed, max_count=65534, extras=0):
    """int32 [n, P + extras, 8] for the plane tests: random records with the boundary grid planted over them (as much of it as fits)"""
    recs = random_records(n * (P + extras), seed, max_count).reshape(n, P + extras, 8).copy()
    grid = boundary_grid()
    if max_count:
        grid = grid[(np.where(grid == ABSENT, 0, grid) <= max_count).all(axis=1)]
    flat = recs[:, :P].reshape(-1, 8)
    k = min(len(grid), len(flat))
    rng = np.random.default_rng(seed + 1)
    flat[rng.choice(len(flat), k, replace=False)] = grid[rng.choice(len(grid), k, replace=False)]
    recs[:, :P] = flat.reshape(n, P, 8)
    recs.setflags(write=False)
    return recs


# the planted cohort: 12 samples of 5 individuals; individual 0 is in both sets, individual 4 among the tumours only
PLANTED_NORMALS = (0, 1, 2, 3, 1, 2, 3)
PLANTED_TUMOURS = (4, 4, 4, 0, 0)


@functools.lru_cache(maxsize=None)
def planted(P=600, seed=14, het=0.15, hom_alt=0.05, error=0.002):
    """recs int32 [12, P, 8] (normals, then tumours) and who [12]: sample -> individual.  An individual is heterozygous at about 15 % of
    the positions and homozygous for another base than the panel's at 5 %; a sample's reads are binomial at depth 300-3000 per position
    with a 0.2 % error spread over the other bases, its strands a fair coin."""
    rng = np.random.default_rng(seed)
    who = np.array(PLANTED_NORMALS + PLANTED_TUMOURS)
    n_ind = int(who.max()) + 1
    ref = rng.integers(0, 4, P)
    u = rng.random((n_ind, P))
    alt = (ref[None, :] + rng.integers(1, 4, (n_ind, P))) % 4
    allele = np.stack([np.where(u < hom_alt, alt, ref[None, :].repeat(n_ind, 0)), np.where(u < hom_alt + het, alt, ref[None, :].repeat(n_ind, 0))], axis=-1)
    recs = np.zeros((len(who), P, 8), np.int32)
    for s, ind in enumerate(who):
        depth = rng.integers(300, 3001, P)
        from_second = rng.binomial(depth, 0.5)
        for p in range(P):
            n = np.zeros(4, np.int64)
            n[allele[ind, p, 0]] += depth[p] - from_second[p]
            n[allele[ind, p, 1]] += from_second[p]
            wrong = rng.binomial(n, error)  # reads of each allele read as another base
            n -= wrong
            for b in range(4):
                if wrong[b]:
                    n += rng.multinomial(wrong[b], [0 if x == b else 1 / 3 for x in range(4)])
            fw = rng.binomial(n, 0.5)
            recs[s, p] = np.concatenate([fw, n - fw])
    recs.setflags(write=False)
    return recs, who


@functools.lru_cache(maxsize=None)
def planted_counts():
    recs, who = planted()
    bits = classify(recs)
    return pair_counts(bits, bits)
