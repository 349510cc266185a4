"""A planted cohort for the false-discovery command line's tests (tests/test_gpu_fdr_cli.py) -- TEST INFRASTRUCTURE.  A panel of normals
and a handful of tumours whose background reads follow one rate (0.1 %) in every cell, and variants planted in the tumours at a few
allele fractions, on both strands."""
import numpy as np

FRACTIONS = (0.003, 0.005, 0.01, 0.02, 0.05)
SEED = 21


def planted(P=300, S=24, T=5, n_var=25, rate=0.001, depth=6000, seed=SEED):
    """normals int32 [S][P][8], tumours int32 [T][P][8], ref_code uint8 [P], variants [(tumour, position, base, fraction)]"""
    rng = np.random.default_rng(seed)
    ref = rng.integers(0, 4, P).astype(np.uint8)

    def files(n):
        d = rng.integers(depth * 3 // 4, depth * 5 // 4, size=(n, P, 2))
        k = rng.poisson(rate * d[:, :, None, :] * np.ones((1, 1, 4, 1)))
        k[:, np.arange(P), ref, :] = 0
        recs = np.zeros((n, P, 8), np.int64)
        for st in range(2):
            recs[:, :, st * 4:st * 4 + 4] = k[:, :, :, st]
            recs[:, np.arange(P), st * 4 + ref] = d[:, :, st] - k[:, :, :, st].sum(axis=2)
        return recs

    normals, tumours = files(S), files(T)
    cells = [(p, b) for p in range(P) for b in range(4) if b != ref[p]]
    variants = []
    for i, c in enumerate(rng.choice(len(cells), n_var, replace=False)):
        p, b = cells[c]
        t, vaf = i % T, FRACTIONS[i % len(FRACTIONS)]
        for st in range(2):
            d = int(tumours[t, p, st * 4:st * 4 + 4].sum())
            add = int(rng.binomial(d, vaf))
            tumours[t, p, st * 4 + b] += add
            tumours[t, p, st * 4 + ref[p]] -= add
        variants.append((t, p, b, vaf))
    assert normals.min() >= 0 and tumours.min() >= 0 and max(normals.max(), tumours.max()) < 65535
    return normals.astype(np.int32), tumours.astype(np.int32), ref, variants
