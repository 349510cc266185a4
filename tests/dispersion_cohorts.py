"""Synthetic panels of normals for the dispersion tests (tests/test_dispersion_model.py, tests/test_gpu_dispersion*.py) -- TEST
INFRASTRUCTURE.  The synthetic generator's normals carry too few alternative reads for a cell to reach K >= 2 at seven normals, so
background reads are drawn on top: a per-(position, base) rate shared by all normals (the null), and at a tenth of the positions a rate
that differs from normal to normal (overdispersed).  Edge-case records, extra occurrences and RD columns as in tests/test_gpu_loo.py."""
import functools

import numpy as np

from tests.helpers import edge_case_recs, synth_recs

ABSENT = np.iinfo(np.int32).min


def cohort(P, S, seed, extras=False, own_rd=False, u16=False, edge=True):
    """recs int32 [S][P+E][8], E, dup_off [P+1], ext_pos [E], rd [S][P+E] or None"""
    rng = np.random.default_rng(seed)
    recs = synth_recs(P, S, seed=0xD15BE25 + seed)
    present = recs[:, :, 0] != ABSENT
    rate = rng.gamma(2.0, 0.0008, size=(1, P, 8))                     # alternative reads at 0.16 % on average
    wild = rng.random(P) < 0.1
    mult = np.where(wild[None, :, None], rng.gamma(0.5, 2.0, size=(S, P, 1)), 1.0)
    depth = np.where(present, recs[:, :, :4].sum(-1), 0)[:, :, None], np.where(present, recs[:, :, 4:].sum(-1), 0)[:, :, None]
    lam = np.concatenate([depth[0] * rate[:, :, :4] * mult, depth[1] * rate[:, :, 4:] * mult], axis=2)
    recs = np.where(present[:, :, None], recs + rng.poisson(lam), recs).astype(np.int32)
    if edge:
        k = max(1, P // 10)
        recs[:, P - k:] = edge_case_recs(k, S, rng)
    E, dup_off, ext_pos = 0, None, None
    if extras:
        m = np.zeros(P, np.int64)
        m[rng.choice(P, max(1, P // 6), replace=False)] = 1
        m[rng.choice(P, max(1, P // 40), replace=False)] = 2
        dup_off = np.concatenate([[0], np.cumsum(m)]).astype(np.uint32)
        E = int(dup_off[-1])
        ext_pos = np.repeat(np.arange(P), m).astype(np.uint32)
        ext = recs[:, ext_pos].copy()  # the same amplicon region read again: close to the primary line, sometimes absent
        ext[:, :, :8] = np.where(ext[:, :, :1] == ABSENT, ext, ext + rng.integers(0, 3, ext.shape).astype(np.int32))
        gone = rng.random((S, E)) < 0.15
        ext[gone] = 0
        ext[gone, 0] = ABSENT
        recs = np.concatenate([recs, ext], axis=1)
    if u16:
        recs = np.where(recs == ABSENT, ABSENT, np.minimum(recs, 65534)).astype(np.int32)
    rd = None
    if own_rd:
        R = P + E
        rd = np.full((S, R), ABSENT, np.int32)
        pick = (rng.random((S, R)) < 0.1) & (recs[:, :, 0] != ABSENT)
        tot = recs.sum(-1)
        rd[pick] = (tot[pick] + rng.integers(0, 50, pick.sum())).astype(np.int32)
    return recs, E, dup_off, ext_pos, rd


def planted(P=200, S=11, seed=5, bad=4, n_planted=20, frac=0.03):
    """11 normals at background; normal `bad` carries `frac` of an alternative base on both strands at n_planted positions.
    Returns recs [S][P][8] and the planted (position, base) pairs."""
    rng = np.random.default_rng(seed)
    recs, _, _, _, _ = cohort(P, S, 1000 + seed, edge=False)
    spots = []
    for p in rng.permutation(P):
        if len(spots) == n_planted:
            break
        if (recs[:, p, 0] == ABSENT).any() or min(recs[bad, p, :4].sum(), recs[bad, p, 4:].sum()) < 500:
            continue
        major = int(np.argmax(recs[bad, p, :4]))
        nt = int((major + 1 + rng.integers(3)) % 4)
        for st in range(2):
            d = int(recs[bad, p, st * 4:st * 4 + 4].sum())
            k = int(d * frac)
            recs[bad, p, st * 4 + major] -= k - int(recs[bad, p, st * 4 + nt])
            recs[bad, p, st * 4 + nt] = k
        spots.append((int(p), nt))
    return recs, spots


@functools.lru_cache(maxsize=None)
def cohort_and_model(P, S, seed, extras, own_rd, u16, cov, z_cutoff=4.0):
    """a cohort with its model, computed once and shared (read only)"""
    from tests.dispersion_model import dispersion_model

    c = cohort(P, S, seed, extras=extras, own_rd=own_rd, u16=u16)
    return c, dispersion_model(c[0], P, cov, E=c[1], ext_pos=c[3], z_cutoff=z_cutoff)
