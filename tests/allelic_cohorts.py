"""Planted cohorts for the allelic-imbalance tests -- TEST INFRASTRUCTURE.

planted(): 24 normals and 6 tumours over P = 600 positions in 12 genes of 50.  About 30 % of the positions carry a SNP (a pair of
bases and a per-position share of the lower base in 0.35 .. 0.65: amplicons amplify alleles unevenly); a sample is het at a SNP with
probability 1/2, so ~15 % of the cells are het sites.  Depths are 1500 .. 2500 reads; reads of a het site are binomial in the
position's share; 0.1 % of the reads of any site are errors.  Tumour PLANT_TUMOUR has its share moved by PLANT_SHIFT = 0.05 over the
het sites of gene PLANT_GENE.  All draws come from numpy's Philox generator."""
import numpy as np

from . import allelic_model as am
from . import concordance_model as cm

ABSENT = np.iinfo(np.int32).min
N_NORMALS, N_TUMOURS, P, GENES, GENE_LEN = 24, 6, 600, 12, 50
PLANT_TUMOUR, PLANT_GENE, PLANT_SHIFT = 2, 4, 0.05


def _records(rng, n, pairs, share, is_snp, shift=None):
    """int32 [n, P, 8] records; shift: float64 [n, P] added to the share of the lower base"""
    Pn = len(is_snp)
    recs = np.zeros((n, Pn, 8), np.int32)
    het = is_snp[None, :] & (rng.random((n, Pn)) < 0.5)
    depth = rng.integers(1500, 2501, (n, Pn))
    err = rng.binomial(depth, 0.001)
    good = depth - err
    sh = np.broadcast_to(share, (n, Pn)) + (0.0 if shift is None else shift)
    k_lo = np.where(het, rng.binomial(good, sh), good)
    k_hi = good - k_lo
    lo, hi = pairs[:, 0], pairs[:, 1]
    tot = np.zeros((n, Pn, 4), np.int64)
    rows, cols = np.meshgrid(np.arange(n), np.arange(Pn), indexing="ij")
    tot[rows, cols, np.broadcast_to(lo, (n, Pn))] += k_lo
    tot[rows, cols, np.broadcast_to(hi, (n, Pn))] += k_hi
    other = (np.broadcast_to(hi, (n, Pn)) + 1 + rng.integers(0, 2, (n, Pn))) % 4  # an error base; it may fall on lo or hi: still an error read
    tot[rows, cols, other] += err
    fw = rng.binomial(tot, 0.5)
    recs[..., :4] = fw
    recs[..., 4:] = tot - fw
    return recs, het


def planted(seed=2025):
    """dict: normals / tumours int32 [n, P, 8], regions (names, reg_off, reg_pos: one per gene and ALL), plant = (tumour, region)"""
    rng = np.random.Generator(np.random.Philox(seed))
    is_snp = rng.random(P) < 0.30
    pairs = np.array(am.PAIRS)[rng.integers(0, 6, P)]
    share = rng.uniform(0.35, 0.65, P)
    normals, _ = _records(rng, N_NORMALS, pairs, share, is_snp)
    shift = np.zeros((N_TUMOURS, P))
    shift[PLANT_TUMOUR, PLANT_GENE * GENE_LEN:(PLANT_GENE + 1) * GENE_LEN] = PLANT_SHIFT
    tumours, _ = _records(rng, N_TUMOURS, pairs, share, is_snp, shift)
    names = [f"GENE{g:02d}" for g in range(GENES)] + ["ALL"]
    lists = [np.arange(g * GENE_LEN, (g + 1) * GENE_LEN) for g in range(GENES)] + [np.arange(P)]
    reg_off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    return dict(normals=normals, tumours=tumours, names=names, reg_off=reg_off, reg_pos=np.concatenate(lists).astype(np.int64),
                plant=(PLANT_TUMOUR, PLANT_GENE), is_snp=is_snp, share=share)


def run_model(co, prm=None):
    """the whole pipeline of the model over a planted cohort, tumours with their own genotypes (pairs=self) and the normals again
    (the null calibration): dict of ref, and per set ("tumours", "normals") the site planes, the sums and the verdicts"""
    prm = dict(am.DEFAULTS, **(prm or {}))
    bits_n = cm.classify(co["normals"])
    ref = am.reference(co["normals"], bits_n, P, prm["min_depth"])
    out = dict(ref=ref)
    for key, bits in (("tumours", cm.classify(co["tumours"])), ("normals", bits_n)):
        recs = co[key]
        q, km, v, code, q64 = am.sites(recs, P, bits, np.arange(len(recs)), ref, prm["min_depth"], prm["min_normals"], True)
        sums = am.region_sums(q, km, v, code, co["reg_off"], co["reg_pos"], prm["site_q"])
        verdicts = [[am.region_verdict(sums[s, r], prm["min_sites"], prm["q_min"], prm["min_imbalance"]) for r in range(sums.shape[1])]
                    for s in range(sums.shape[0])]
        out[key] = dict(q=q, km=km, v=v, code=code, q64=q64, sums=sums, verdicts=verdicts)
    return out


def small(P_, n, seed, layout_max=None, absent=0.05, deep=False):
    """a small random chunk for the kernels' tests: int32 [n, P_, 8] records with het sites (all six pairs), absent records, shallow
    cells and -- with deep -- int32 depths beyond 2^22 and 2^30 and cells beyond 2^31 - 1.  layout_max caps every count (65534 for
    uint16 records)."""
    rng = np.random.Generator(np.random.Philox(seed))
    is_snp = rng.random(P_) < 0.5
    pairs = np.array(am.PAIRS)[rng.integers(0, 6, P_)]
    share = rng.uniform(0.35, 0.65, P_)
    recs, _ = _records(rng, n, pairs, share, is_snp)
    sel = rng.random((n, P_)) < 0.15  # shallow cells around min_depth = 100
    scale = rng.choice([0.03, 0.0497, 0.05, 0.0503, 0.08], (n, P_))
    recs = np.where(sel[..., None], (recs * scale[..., None]).astype(np.int32), recs)
    if deep:
        big = rng.random((n, P_)) < 0.10
        mult = rng.choice([1 << 12, 1 << 19, (1 << 20) - 1, 1 << 20], (n, P_))
        recs = np.where(big[..., None], np.minimum(recs.astype(np.int64) * mult[..., None], 2 ** 31 - 1).astype(np.int32), recs)
    if layout_max is not None:
        recs = np.minimum(recs, layout_max)
    gone = rng.random((n, P_)) < absent
    recs[gone] = 0
    recs[gone, 0] = ABSENT
    return recs
