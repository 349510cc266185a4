"""The planted cohort of the exceedance tests (tests/test_exceedance_*.py, tests/test_gpu_exceedance*.py) -- TEST INFRASTRUCTURE.
Everything is drawn once with a fixed seed and shared read-only.

The panel: 16 runs of 100-150 consecutive coordinates on four chromosomes (P about 2000), reference bases uniform over A C G T, two
positions with N and one with a lower-case base (neither is a reference base: their cells are NA).  The background: one rate per
(position, alternative base) drawn once from 2e-4 .. 1e-3, the same for every file and both strands, so that a clean tumour is
exchangeable with the normals.  24 normals: a depth of 500-5000 per strand and position, Poisson alternative counts, 1 % of the records
absent; at each of 5 "het" positions two normals are heterozygous (45-55 % of both strands on one alternative).  Five tumours:
  T_CLEAN   clean
  T_VAR     clean, with 40 variants of 5 % of both strands on positions no normal is polymorphic at
  T_HET     clean, with a variant of 5 % at each of the 5 het positions, on the normals' alternative
  T_SHALLOW 5-60 reads per strand: below the calling cut-off everywhere
  T_NONE    no line at all (a header-only file)"""
import functools

import numpy as np

from tests.exceedance_model import ABSENT, DEFAULTS, NT, candidates, exceedance

N_NORMALS = 24
TUMOURS = ("TCLEAN", "TVAR", "THET", "TSHALLOW", "TNONE")
T_CLEAN, T_VAR, T_HET, T_SHALLOW, T_NONE = range(N_NORMALS, N_NORMALS + len(TUMOURS))
NAMES = [f"N{i:02d}" for i in range(N_NORMALS)] + list(TUMOURS)
CHROMS = ("chr1", "chr2", "chr7", "chr17")
RUNS = 16
N_VAR, N_HET, VAF = 40, 5, 0.05
CAND = {k: DEFAULTS[k] for k in ("min_alt_reads", "min_vaf_pm", "min_normals", "max_normals")}


@functools.lru_cache(maxsize=None)
def planted(seed=18):
    """dict: recs int32 [29, P, 8] (normals, then tumours), P, positions [(chrom, coordinate)], bases {(chrom, coordinate): str},
    ref_code uint8 [P], variants [(position index, alternative)] x 40 of T_VAR, hets [(position index, alternative)] x 5 of T_HET"""
    rng = np.random.default_rng(seed)
    positions, bases = [], {}
    for k in range(RUNS):
        first, n = 100000 * (k // len(CHROMS) + 1), int(rng.integers(100, 151))
        positions += [(CHROMS[k % len(CHROMS)], first + i) for i in range(n)]
    P = len(positions)
    letters = rng.integers(0, 4, P)
    for p, pos in enumerate(positions):
        bases[pos] = NT[letters[p]]
    odd = rng.choice(P, 3, replace=False)
    for p in odd[:2]:
        bases[positions[p]] = "N"
    bases[positions[odd[2]]] = NT[letters[odd[2]]].lower()
    ref_code = np.array([NT.index(bases[pos]) if bases[pos] in tuple(NT) else 255 for pos in positions], np.uint8)
    S = N_NORMALS + len(TUMOURS)
    r = letters.astype(np.int64)                       # the base the reads are on, a reference base or not
    rate = rng.uniform(2e-4, 1e-3, (P, 4))
    depth = rng.integers(500, 5001, (S, 2, P))
    depth[T_SHALLOW] = rng.integers(5, 61, (2, P))
    recs = np.zeros((S, P, 8), np.int64)
    for s in range(S):
        for st in range(2):
            k = rng.poisson(depth[s, st][:, None] * rate)
            k[np.arange(P), r] = 0
            recs[s, :, 4 * st:4 * st + 4] = k
            recs[s, np.arange(P), 4 * st + r] = depth[s, st] - k.sum(1)

    def move(s, p, y, share):  # reads from the base the position's reads are on to y, on both strands
        for st in range(2):
            k = int(round(depth[s, st, p] * share))
            recs[s, p, 4 * st + r[p]] -= k
            recs[s, p, 4 * st + y] += k

    sites = rng.choice(np.setdiff1d(np.arange(P), odd), N_VAR + N_HET, replace=False)
    variants = [(int(p), int((r[p] + 1 + i % 3) % 4)) for i, p in enumerate(sites[:N_VAR])]
    hets = [(int(p), int((r[p] + 1 + i % 3) % 4)) for i, p in enumerate(sites[N_VAR:])]
    for p, y in variants:
        move(T_VAR, p, y, VAF)
    for i, (p, y) in enumerate(hets):
        move(T_HET, p, y, VAF)
        for s in rng.choice(N_NORMALS, 2, replace=False):
            move(int(s), p, y, float(rng.uniform(0.45, 0.55)))
    gone = rng.random((S, P)) < 0.01
    gone[:, sites] = False                             # every planted record is there
    gone[T_NONE] = True
    recs[gone] = 0
    recs[gone, 0] = ABSENT
    assert recs.max() <= 65534 and recs[~gone].min() >= 0
    recs = recs.astype(np.int32)
    for v in (recs, ref_code):
        v.setflags(write=False)
    return dict(recs=recs, P=P, positions=positions, bases=bases, ref_code=ref_code, variants=variants, hets=hets)


@functools.lru_cache(maxsize=None)
def planted_results():
    """the model's counts and candidates of the planted cohort at the default parameters: the tumours against the 24 normals (elig, ge,
    cand: rows T_CLEAN - 24 ...), and the normals against themselves without the file's own row (self_elig, self_ge, self_cand)"""
    c = planted()
    n, t = c["recs"][:N_NORMALS], c["recs"][N_NORMALS:]
    cut = dict(normal_cutoff=DEFAULTS["coverage_cutoff"], calling_cutoff=DEFAULTS["calling_cutoff"])
    elig, ge = exceedance(t, n, c["ref_code"], first_t=N_NORMALS, **cut)
    self_elig, self_ge = exceedance(n, n, c["ref_code"], skip_same_index=True, **cut)
    out = dict(elig=elig, ge=ge, cand=candidates(t, elig, ge, **CAND), self_elig=self_elig, self_ge=self_ge, self_cand=candidates(n, self_elig, self_ge, **CAND))
    for v in out.values():
        v.setflags(write=False)
    return out
