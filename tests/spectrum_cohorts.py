"""The planted cohort of the substitution spectrum tests (tests/test_spectrum_*.py, tests/test_gpu_spectrum*.py) -- TEST INFRASTRUCTURE.
Everything is drawn once with a fixed seed and shared read-only.

The panel: 24 runs of 90-160 consecutive coordinates on six chromosomes (P about 3000), reference bases uniform over A C G T, three
positions with N and one with a lower-case base (not a reference base itself, but a valid neighbour).  A run's first and last position
have no trinucleotide class.  The background: one rate per strand-resolved type drawn once from 2e-4 .. 1e-3, the same on both strands.
12 normals: a per-file factor of 0.7-1.4 on every rate, a depth of 250-2500 per strand and position, Poisson alternative counts, 1 % of
the records absent.  Six tumours, all with factor 1:
  T_DEAM    C>T and G>A at 5 x
  T_OXFW    G>T at 4 x on the forward strand only
  T_CLEAN   clean, at 3 x the depth
  T_VAR     clean, with 30 heterozygous and 10 somatic 20 % positions, which the gate must keep out
  T_SHALLOW 5-40 reads per strand except on 160 positions: fewer than min_sites sites per reference base
  T_NONE    no line at all (a header-only file)"""
import functools

import numpy as np

from tests.spectrum_model import ABSENT, CLASSES, DEFAULTS, NT, TYPES, class_sums, fold, panel_classes, score

N_NORMALS = 12
TUMOURS = ("TDEAM", "TOXFW", "TCLEAN", "TVAR", "TSHALLOW", "TNONE")
T_DEAM, T_OXFW, T_CLEAN, T_VAR, T_SHALLOW, T_NONE = range(N_NORMALS, N_NORMALS + len(TUMOURS))
NAMES = [f"N{i:02d}" for i in range(N_NORMALS)] + list(TUMOURS)
CHROMS = ("chr1", "chr2", "chr3", "chr7", "chr12", "chr17")
RUNS = 24
TY = {f"{NT[r]}>{NT[y]}": 3 * r + (y if y < r else y - 1) for r in range(4) for y in range(4) if y != r}
PLANTED = {T_DEAM: {TY["C>T"]: (5.0, 5.0), TY["G>A"]: (5.0, 5.0)}, T_OXFW: {TY["G>T"]: (4.0, 1.0)}}  # type -> factor on (fw, bw)


@functools.lru_cache(maxsize=None)
def planted(seed=17):
    """dict: recs int32 [18, P, 8] (normals, then tumours), P, positions [(chrom, coordinate)], bases {(chrom, coordinate): str},
    ref_code, cls uint8 [P], rate float64 [12] (the background), factor float64 [18], variants (the positions of T_VAR's variants)"""
    rng = np.random.default_rng(seed)
    positions, bases = [], {}
    for k in range(RUNS):
        first, n = 100000 * (k // len(CHROMS) + 1), int(rng.integers(90, 161))
        positions += [(CHROMS[k % len(CHROMS)], first + i) for i in range(n)]
    P = len(positions)
    letters = rng.integers(0, 4, P)
    for p, pos in enumerate(positions):
        bases[pos] = NT[letters[p]]
    odd = rng.choice(np.arange(5, P - 5), 4, replace=False)
    for p in odd[:3]:
        bases[positions[p]] = "N"
    bases[positions[odd[3]]] = NT[letters[odd[3]]].lower()
    ref_code, cls = panel_classes(positions, bases)
    S = N_NORMALS + len(TUMOURS)
    rate = rng.uniform(2e-4, 1e-3, 12)
    factor = np.concatenate([rng.uniform(0.7, 1.4, N_NORMALS), np.ones(len(TUMOURS))])
    depth = rng.integers(250, 2501, (S, 2, P))
    depth[T_CLEAN] *= 3
    deep = rng.choice(P, 160, replace=False)
    shallow = rng.integers(5, 41, (2, P))
    shallow[:, deep] = depth[T_SHALLOW][:, deep]
    depth[T_SHALLOW] = shallow
    r = np.where(ref_code <= 3, ref_code, letters).astype(np.int64)  # a position that is not a reference base still has reads
    recs = np.zeros((S, P, 8), np.int64)
    for s in range(S):
        for st in range(2):
            alts = np.zeros(P, np.int64)
            for y in range(4):
                ty = 3 * r + np.where(y < r, y, y - 1)
                lam = depth[s, st] * rate[np.clip(ty, 0, 11)] * factor[s]
                for t, mult in PLANTED.get(s, {}).items():
                    lam = np.where(ty == t, lam * mult[st], lam)
                k = np.where(y == r, 0, rng.poisson(lam))
                recs[s, :, 4 * st + y] = k
                alts += k
            recs[s, np.arange(P), 4 * st + r] = depth[s, st] - alts
    variants = rng.choice(np.flatnonzero(cls < 64), 40, replace=False)
    for i, p in enumerate(variants):  # 30 hets at about 50 %, 10 somatic at about 20 %: reads move from the reference base to another
        y = (r[p] + 1 + i % 3) % 4
        for st in range(2):
            k = int(recs[T_VAR, p, 4 * st + r[p]] * (0.5 if i < 30 else 0.2))
            recs[T_VAR, p, 4 * st + r[p]] -= k
            recs[T_VAR, p, 4 * st + y] += k
    gone = rng.random((S, P)) < 0.01
    gone[T_NONE] = True
    recs[gone] = 0
    recs[gone, 0] = ABSENT
    assert recs.max() <= 65534 and recs[~gone].min() >= 0
    recs = recs.astype(np.int32)
    for v in (recs, ref_code, cls, rate, factor, variants):
        v.setflags(write=False)
    return dict(recs=recs, P=P, positions=positions, bases=bases, ref_code=ref_code, cls=cls, rate=rate, factor=factor, variants=variants)


@functools.lru_cache(maxsize=None)
def planted_results():
    """the model's sums, fold and score of the planted cohort at the default parameters"""
    c = planted()
    sums = class_sums(c["recs"], c["ref_code"], c["cls"], CLASSES, DEFAULTS["coverage_cutoff"], DEFAULTS["max_alt_pm"])
    f = fold(sums)
    sc = score(f, N_NORMALS, **{k: DEFAULTS[k] for k in ("min_sites", "min_normals", "excess_ratio", "z_cutoff", "asym_delta")})
    sums.setflags(write=False)
    assert sc["flag"].shape == (len(NAMES), TYPES)
    return dict(sums=sums, fold=f, score=sc)
