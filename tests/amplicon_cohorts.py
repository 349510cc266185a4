"""The planted cohort of the amplicon coverage tests (tests/test_amplicon_*.py, tests/test_gpu_amplicon*.py) -- TEST INFRASTRUCTURE.
Everything is drawn once with a fixed seed and shared read-only.

40 amplicons of 60-200 positions in 8 genes of 5 (G0 .. G5 autosomal, X0 and X1 on chrX); amplicons 7 and 8 overlap by 20 positions.
12 normals: library size 0.5-2x, a fixed efficiency of 0.3-3x per amplicon, Poisson counts per strand (400 reads per strand at
efficiency 1 and library size 1), every second normal with half the depth on chrX, amplicon 13 at zero in every file, 1 % of the records
absent.  Five tumours: T0 gene G1 at 2x, T1 gene G2 at 0.5x, T2 clean at 3x library size, T3 amplicon 21 (gene G4) dropped out to 5 %,
T4 clean with half depth on chrX."""
import functools

import numpy as np

from tests.amplicon_model import ABSENT, DEFAULTS, depth_sums, genes, ratios, reference

N_NORMALS, N_TUMOURS, PER_GENE = 12, 5, 5
GENES = ("G0", "G1", "G2", "G3", "G4", "G5", "X0", "X1")
CHROMS = ("chr1", "chr2", "chr3", "chr7", "chr12", "chr17", "chrX", "chrX")
A = len(GENES) * PER_GENE
OVERLAP = (7, 8, 20)  # amplicon 8 starts 20 positions before amplicon 7 ends
ZERO_AMPLICON, DROPPED_AMPLICON, DROPPED_TO = 13, 21, 0.05
GAIN_GENE, LOSS_GENE = "G1", "G2"
T_GAIN, T_LOSS, T_BIG, T_DROP, T_MALE = range(N_NORMALS, N_NORMALS + N_TUMOURS)
BASE = 400  # reads per strand and position at efficiency 1, library size 1


def lists_from_cover(spans, P):
    """the amplicons' lists as the command line builds them: amplicon a's positions that no other amplicon covers (all of them if that
    leaves none).  spans: [(first position, length)].  Returns amp_off, amp_pos."""
    cover = np.zeros(P, np.int64)
    for lo, n in spans:
        cover[lo:lo + n] += 1
    off, pos = [0], []
    for lo, n in spans:
        own = [p for p in range(lo, lo + n) if cover[p] == 1] or list(range(lo, lo + n))
        pos += own
        off.append(len(pos))
    return np.array(off, np.uint32), np.array(pos, np.uint32)


@functools.lru_cache(maxsize=None)
def planted(seed=16):
    """dict: recs int32 [17, P, 8] (normals, then tumours), spans, amp_off, amp_pos, gene_of [A], chrom_of [A], use uint8 [A] (0 on
    chrX), planted float64 [17, A] (the copy ratio every file was drawn with, relative to a female normal), lib [17]"""
    rng = np.random.default_rng(seed)
    length = rng.integers(60, 201, A)
    spans, p = [], 0
    for a in range(A):
        if a == OVERLAP[1]:
            p -= OVERLAP[2]
        spans.append((p, int(length[a])))
        p += int(length[a])
    P = p
    gene_of = [GENES[a // PER_GENE] for a in range(A)]
    chrom_of = [CHROMS[a // PER_GENE] for a in range(A)]
    on_x = np.array([c == "chrX" for c in chrom_of])
    eff = rng.uniform(0.3, 3.0, A)
    eff[ZERO_AMPLICON] = 0.0
    S = N_NORMALS + N_TUMOURS
    lib = np.concatenate([rng.uniform(0.5, 2.0, N_NORMALS), rng.uniform(0.7, 1.5, N_TUMOURS)])
    lib[T_BIG] = 3.0
    cn = np.ones((S, A))
    cn[1:N_NORMALS:2, on_x] = 0.5  # every second normal is male
    cn[T_GAIN, [g == GAIN_GENE for g in gene_of]] = 2.0
    cn[T_LOSS, [g == LOSS_GENE for g in gene_of]] = 0.5
    cn[T_DROP, DROPPED_AMPLICON] = DROPPED_TO
    cn[T_MALE, on_x] = 0.5
    lam = np.zeros((S, P))
    for a, (lo, n) in enumerate(spans):
        lam[:, lo:lo + n] += (lib[:, None] * cn[:, a:a + 1] * eff[a] * BASE)
    ref_base = rng.integers(0, 4, P)
    recs = np.zeros((S, P, 8), np.int32)
    fw, bw = rng.poisson(lam), rng.poisson(lam)
    recs[:, np.arange(P), ref_base] = fw
    recs[:, np.arange(P), 4 + ref_base] = bw
    gone = rng.random((S, P)) < 0.01
    recs[gone] = 0
    recs[gone, 0] = ABSENT
    assert recs.max() <= 65534
    amp_off, amp_pos = lists_from_cover(spans, P)
    use = (~on_x).astype(np.uint8)
    for v in (recs, amp_off, amp_pos, use, cn, lib):
        v.setflags(write=False)
    return dict(recs=recs, P=P, spans=spans, amp_off=amp_off, amp_pos=amp_pos, gene_of=gene_of, chrom_of=chrom_of, use=use, planted=cn, lib=lib)


@functools.lru_cache(maxsize=None)
def planted_results():
    """the model's sums, reference, ratios and genes of the planted cohort at the default parameters"""
    c = planted()
    sums = depth_sums(c["recs"], c["amp_off"], c["amp_pos"], DEFAULTS["coverage_cutoff"])
    ref = reference(sums[:N_NORMALS], c["use"], DEFAULTS["min_normals"])
    rat = ratios(sums, c["use"], ref)
    kw = {k: DEFAULTS[k] for k in ("min_amplicons", "gain_ratio", "loss_ratio", "z_cutoff")}
    g = genes(rat["ratio"], rat["z"], ref["status"], c["gene_of"], **kw)
    sums.setflags(write=False)
    return dict(sums=sums, ref=ref, rat=rat, genes=g)
