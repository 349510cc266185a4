"""The definition of the sample-identity check in plain numpy -- TEST INFRASTRUCTURE, the yardstick of
ampli_genotype_classify, genotype_planes_kernel, concordance_pairs_kernel and AmpliSolveSampleConcordance.

Genotypes come from int64 arithmetic on the int32 records (1000 n < 2^45 for any record).  The pair counts come from matrix products
of one-hot indicator matrices (one per presence set), not from bit tricks: the model and the kernel share nothing.  The products run
in float64, where sums of at most P < 2^31 ones are exact integers."""
import numpy as np

ABSENT = np.iinfo(np.int32).min
DEFAULTS = dict(min_depth=100, absent_max_pm=100, het_min_pm=250, het_max_pm=750, hom_min_pm=900)
V, A, C, G, T, H = 1, 2, 4, 8, 16, 32  # AMPLI_GENO_*: bit k is plane k
UNDETERMINED, SAME, DIFFERENT = 0, 1, 2
RELATION = ("UNDETERMINED", "SAME", "DIFFERENT")


def params_ok(min_depth, absent_max_pm, het_min_pm, het_max_pm, hom_min_pm):
    return min_depth >= 1 and 0 <= absent_max_pm < het_min_pm <= het_max_pm < hom_min_pm <= 1000


def classify(recs, min_depth=100, absent_max_pm=100, het_min_pm=250, het_max_pm=750, hom_min_pm=900):
    """int32 [..., 8] records (absent: field 0 == INT32_MIN) -> uint8 [...] plane bits"""
    assert params_ok(min_depth, absent_max_pm, het_min_pm, het_max_pm, hom_min_pm)
    r = np.asarray(recs).astype(np.int64)
    present = r[..., 0] != ABSENT
    n = np.where(present[..., None], r[..., :4] + r[..., 4:], 0)
    d = n.sum(-1)[..., None]
    k = 1000 * n
    absent = k <= absent_max_pm * d
    het = (k >= het_min_pm * d) & (k <= het_max_pm * d)
    hom = k >= hom_min_pm * d
    n_het, n_hom, n_amb = het.sum(-1), hom.sum(-1), (~(absent | het | hom)).sum(-1)
    valid = present & (d[..., 0] >= min_depth) & (n_amb == 0) & (((n_hom == 1) & (n_het == 0)) | ((n_het == 2) & (n_hom == 0)))
    bits = np.zeros(r.shape[:-1], np.int64)
    for b in range(4):
        bits |= (het[..., b] | hom[..., b]).astype(np.int64) << (b + 1)
    bits |= 1 | ((n_het == 2).astype(np.int64) << 5)
    return np.where(valid, bits, 0).astype(np.uint8)


def words(P):
    return (P + 63) // 64


def pack_planes(bits, P):
    """uint8 [S, >= P] plane bits of the primary records -> uint64 [S, 6, W]: bit i of word w is position 64 w + i"""
    S, W = bits.shape[0], words(P)
    out = np.zeros((S, 6, W), np.uint64)
    weight = np.uint64(1) << np.arange(64, dtype=np.uint64)
    for k in range(6):
        b = np.zeros((S, W * 64), np.uint64)
        b[:, :P] = (bits[:, :P] >> k) & 1
        out[:, k] = (b.reshape(S, W, 64) * weight).sum(-1, dtype=np.uint64)
    return out


def planes(recs, P, **prm):
    """int32 [S, P + E, 8] -> uint64 [S, 6, W]; only the primary records (slot r < P) enter"""
    return pack_planes(classify(np.asarray(recs)[:, :P], **prm), P)


def pair_counts(bits_a, bits_b):
    """uint8 [n_a, P], [n_b, P] plane bits -> int32 [n_a, n_b, 5]: sites, match, ibs0, het_either, het_match"""
    va, vb = (bits_a & V) != 0, (bits_b & V) != 0
    sa, sb = (bits_a >> 1) & 15, (bits_b >> 1) & 15  # the presence set of a valid position: one or two bases
    ha, hb = (bits_a & H) != 0, (bits_b & H) != 0
    f = lambda m: m.astype(np.float64)
    sites = f(va) @ f(vb).T
    match = np.zeros_like(sites)
    het_match = np.zeros_like(sites)
    share = np.zeros_like(sites)
    codes = [c for c in range(1, 16) if bin(c).count("1") in (1, 2)]
    for c in codes:
        oa = f(va & (sa == c))
        same = oa @ f(vb & (sb == c)).T  # on a valid position the presence set fixes the genotype
        match += same
        if bin(c).count("1") == 2:
            het_match += same
        shares_c = np.array([(c & x) != 0 for x in range(16)])
        share += oa @ f(vb & shares_c[sb]).T
    het_either = f(ha) @ f(vb).T + f(va) @ f(hb).T - f(ha) @ f(hb).T  # H is 0 where V is 0
    out = np.stack([sites, match, sites - share, het_either, het_match], axis=-1)
    assert (out == np.rint(out)).all() and (out >= 0).all()
    return out.astype(np.int32)


def relation(het_either, het_match, min_sites, same_fraction):
    if het_either < min_sites:
        return UNDETERMINED
    return SAME if float(het_match) >= same_fraction * float(het_either) else DIFFERENT


def relations(counts, min_sites, same_fraction):
    n_a, n_b = counts.shape[:2]
    return np.array([[relation(int(counts[i, j, 3]), int(counts[i, j, 4]), min_sites, same_fraction) for j in range(n_b)] for i in range(n_a)])


def format_files(names, n_normals, counts, min_sites, same_fraction, prm=None):
    """the three files of AmpliSolveSampleConcordance from the N x N counts of normals-then-tumours: (samples, pairs, summary)"""
    prm = dict(DEFAULTS, **(prm or {}))
    N = len(names)
    c = counts.astype(np.int64)
    rel = relations(counts, min_sites, same_fraction)
    samples = "Sample\tSet\tValidSites\tHetSites\tSamePartners\tNearest\tNearestHetEither\tNearestHetMatch\tNearestConcordance\n"
    for i in range(N):
        same = sum(1 for j in range(N) if j != i and rel[i, j] == SAME)
        best = -1
        for j in range(N):
            if j == i or rel[i, j] == UNDETERMINED:
                continue
            if best < 0 or int(c[i, j, 4]) * int(c[i, best, 3]) > int(c[i, best, 4]) * int(c[i, j, 3]):  # fractions of integers; the first wins a tie
                best = j
        samples += f"{names[i]}\t{'N' if i < n_normals else 'T'}\t{c[i, i, 0]}\t{c[i, i, 3]}\t{same}\t"
        samples += "NA\tNA\tNA\tNA\n" if best < 0 else f"{names[best]}\t{c[i, best, 3]}\t{c[i, best, 4]}\t{'%.4f' % (float(c[i, best, 4]) / float(c[i, best, 3]))}\n"
    pairs = "SampleA\tSampleB\tSites\tMatch\tIBS0\tHetEither\tHetMatch\tConcordance\tRelation\n"
    by = [0, 0, 0]
    for i in range(N):
        for j in range(i + 1, N):
            by[rel[i, j]] += 1
            if rel[i, j] == DIFFERENT:
                continue
            conc = "%.4f" % (float(c[i, j, 4]) / float(c[i, j, 3])) if c[i, j, 3] > 0 else "NA"
            pairs += f"{names[i]}\t{names[j]}\t" + "\t".join(str(int(x)) for x in c[i, j]) + f"\t{conc}\t{RELATION[rel[i, j]]}\n"
    summary = (f"normals={n_normals}\ntumours={N - n_normals}\n" + "".join(f"{k}={prm[k]}\n" for k in DEFAULTS) +
               f"min_sites={min_sites}\nsame_fraction={'%g' % same_fraction}\npairs_same={by[SAME]}\npairs_different={by[DIFFERENT]}\n"
               f"pairs_undetermined={by[UNDETERMINED]}\n")
    return samples, pairs, summary
