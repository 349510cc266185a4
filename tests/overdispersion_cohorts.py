"""Planted cohorts for the overdispersion tests (tests/test_overdispersion_*.py, tests/test_gpu_overdispersion*.py) -- TEST
INFRASTRUCTURE.  A panel of normals whose background reads follow one rate per cell, except at `n_over` (position, base) cells where
the rate is higher and differs from file to file (one gamma factor of mean 1 and variance omega per file, shared by the strands); tumours with the same background -- the
overdispersed cells included -- and variants at 2 % planted on ordinary and on overdispersed cells."""
import functools

import numpy as np

ABSENT = np.iinfo(np.int32).min
C_VALUE = 0.002
Z_CUTOFF = 4.0
COV = 100


def planted(P=200, S=32, T=4, n_over=30, n_var=16, n_var_over=6, omega=1.5, rate=0.001, rate_over=0.004, vaf=0.02, depth=6000, seed=19):
    """normals int32 [S][P][8], tumours int32 [T][P][8], ref_code uint8 [P], over: the overdispersed (position, base) pairs,
    variants: (tumour, position, base, on an overdispersed cell)"""
    rng = np.random.default_rng(seed)
    ref = rng.integers(0, 4, P).astype(np.uint8)
    cells = [(p, b) for p in range(P) for b in range(4) if b != ref[p]]
    pick = rng.choice(len(cells), n_over, replace=False)
    over = [cells[i] for i in pick]
    over_set = set(over)

    def files(n):
        d = rng.integers(depth * 3 // 4, depth * 5 // 4, size=(n, P, 2))  # unequal depths: D - S2 / D is not D (1 - 1 / n)
        lam = np.full((n, P, 4, 2), rate)
        for p, b in over:
            lam[:, p, b, :] = rate_over * rng.gamma(1.0 / omega, omega, size=(n, 1))  # a noisy site: one factor per file, both strands
        k = rng.poisson(lam * d[:, :, None, :])
        k[:, np.arange(P), ref, :] = 0
        recs = np.zeros((n, P, 8), np.int64)
        for st in range(2):
            recs[:, :, st * 4:st * 4 + 4] = k[:, :, :, st]
            recs[:, np.arange(P), st * 4 + ref] = d[:, :, st] - k[:, :, :, st].sum(axis=2)
        return recs

    normals, tumours = files(S), files(T)
    ordinary = [c for c in cells if c not in over_set]
    spots = [ordinary[i] for i in rng.choice(len(ordinary), n_var, replace=False)] + [over[i] for i in rng.choice(n_over, n_var_over, replace=False)]
    variants = []
    for i, (p, b) in enumerate(spots):
        t = i % T
        for st in range(2):
            d = int(tumours[t, p, st * 4:st * 4 + 4].sum())
            add = int(rng.binomial(d, vaf))
            tumours[t, p, st * 4 + b] += add
            tumours[t, p, st * 4 + ref[p]] -= add
        variants.append((t, p, b, (p, b) in over_set))
    assert normals.min() >= 0 and tumours.min() >= 0 and max(normals.max(), tumours.max()) < 65535
    return normals.astype(np.int32), tumours.astype(np.int32), ref, over, variants


def stand_in_thr(K, D, C=C_VALUE):
    """a threshold table for the tests that have no device: the pooled rate K / D of the C = 0 sums plus C (what sum (k_i + C d_i) /
    sum d_i of the error estimation comes to), C alone where the cell has no depth, as float32 [2][4][P].  The score takes whatever
    table it is given."""
    r = np.where(D > 0, K / np.maximum(D, 1), 0.0)
    return (r + C).astype(np.float32)


@functools.lru_cache(maxsize=None)
def planted_and_fit(**kw):
    """the planted cohort with the model's fit of its panel: (normals, tumours, ref, over, variants), the dispersion model's planes,
    S2 (integers), omega and its bound -- computed once and shared (read only)"""
    from tests.dispersion_model import dispersion_model
    from tests.overdispersion_model import omega_model, s2_model

    c = planted(**kw)
    P = c[0].shape[1]
    dm = dispersion_model(c[0], P, COV, z_cutoff=Z_CUTOFF)
    s2 = s2_model(c[0], P, COV)
    w, bound = omega_model(dm["status"], dm["n"], dm["K"], dm["D"], dm["x2"], s2)
    return c, dm, s2, w, bound


def tally(q0, q, q_min, over, variants):
    """what Overdispersed_Samples.txt counts, from the two score arrays [T][P][4][2]: cells passing Poisson and passing both among the
    background cells at overdispersed sites, the ordinary background cells, and the variants"""
    pass0 = (q0[..., 0] >= q_min) & (q0[..., 1] >= q_min)
    pass1 = pass0 & (q[..., 0] >= q_min) & (q[..., 1] >= q_min)
    is_var = np.zeros(pass0.shape, bool)
    for t, p, b, _ in variants:
        is_var[t, p, b] = True
    at_over = np.zeros(pass0.shape, bool)
    for p, b in over:
        at_over[:, p, b] = True
    bg = ~is_var
    return dict(over_poisson=int((pass0 & bg & at_over).sum()), over_kept=int((pass1 & bg & at_over).sum()),
                ordinary_poisson=int((pass0 & bg & ~at_over).sum()), ordinary_kept=int((pass1 & bg & ~at_over).sum()),
                var_ordinary_kept=[bool(pass1[t, p, b]) for t, p, b, o in variants if not o],
                var_over_poisson=int(sum(pass0[t, p, b] for t, p, b, o in variants if o)),
                var_over_kept=int(sum(pass1[t, p, b] for t, p, b, o in variants if o)))
