"""The planted cohort of the contamination tests (tests/test_contamination_*.py, tests/test_gpu_contamination*.py) -- TEST
INFRASTRUCTURE: six synthetic individuals, one clean sample of each, then six mixtures in which a fraction c of a recipient's reads
comes from a source individual.  The individuals follow the recipe of tests/concordance_cohorts.planted -- its panel size, seed, het
and hom-alt shares and error rate are read off that function's signature, and the three draws (reference base, genotype class, other
base) are made in its order -- with six individuals instead of five.  Everything is computed once and shared read-only."""
import functools
import inspect

import numpy as np

from tests.concordance_cohorts import planted as _recipe
from tests.concordance_model import classify
from tests.contamination_model import sums

_PRM = {k: v.default for k, v in inspect.signature(_recipe.__wrapped__).parameters.items()}  # P, seed, het, hom_alt, error
N_INDIVIDUALS = 6
# (recipient, source, c): sample 6 + k is mostly individual `recipient`; (3, 3, 0.05) is a sample mixed with itself
MIXTURES = ((0, 1, 0.01), (2, 3, 0.03), (4, 5, 0.08), (1, 0, 0.002), (3, 3, 0.05), (5, 2, 0.15))
WHO = tuple(range(N_INDIVIDUALS)) + tuple(m[0] for m in MIXTURES)  # sample -> the individual most of its reads come from


def _individuals(rng, P, n_ind, het, hom_alt):
    """allele int [n_ind, P, 2]: the two alleles of every individual at every position (the recipe's draws, in its order)"""
    ref = rng.integers(0, 4, P)
    u = rng.random((n_ind, P))
    alt = (ref[None, :] + rng.integers(1, 4, (n_ind, P))) % 4
    refs = ref[None, :].repeat(n_ind, 0)
    return np.stack([np.where(u < hom_alt, alt, refs), np.where(u < hom_alt + het, alt, refs)], axis=-1)


def _reads(rng, allele, depth, error):
    """n int64 [P, 4]: `depth` reads of one individual, a fair coin between its two alleles, `error` of each allele's reads spread over
    the other three bases"""
    P = len(depth)
    rows = np.arange(P)
    second = rng.binomial(depth, 0.5)
    n = np.zeros((P, 4), np.int64)
    np.add.at(n, (rows, allele[:, 0]), depth - second)
    np.add.at(n, (rows, allele[:, 1]), second)
    wrong = rng.binomial(n, error)
    n -= wrong
    for b in range(4):
        n += rng.multinomial(wrong[:, b], [0 if x == b else 1 / 3 for x in range(4)])
    return n


@functools.lru_cache(maxsize=None)
def planted():
    """recs int32 [12, P, 8] and who [12]: depth 300-3000 per position, of which Binomial(depth, c) reads are the source's"""
    P, error = _PRM["P"], _PRM["error"]
    rng = np.random.default_rng(_PRM["seed"])
    allele = _individuals(rng, P, N_INDIVIDUALS, _PRM["het"], _PRM["hom_alt"])
    plan = [(i, i, 0.0) for i in range(N_INDIVIDUALS)] + list(MIXTURES)
    recs = np.zeros((len(plan), P, 8), np.int32)
    for s, (own, src, c) in enumerate(plan):
        depth = rng.integers(300, 3001, P)
        foreign = rng.binomial(depth, c)
        n = _reads(rng, allele[own], depth - foreign, error) + _reads(rng, allele[src], foreign, error)
        fw = rng.binomial(n, 0.5)
        recs[s] = np.concatenate([fw, n - fw], axis=1)
    recs.setflags(write=False)
    return recs, np.array(WHO)


@functools.lru_cache(maxsize=None)
def planted_sums():
    recs, _ = planted()
    bits = classify(recs)
    out = sums(recs, bits, bits)
    out.setflags(write=False)
    return out
