"""The definition of allelic imbalance at germline het sites in numpy, float64 / int64 -- TEST INFRASTRUCTURE, and the text
that include/amplisolve_hip.h, include/amplisolve_host.h, csrc/ampli_math.h and csrc/ampli_allelic.hip restate.

Bases A, C, G, T = 0..3; pair code c = 0..5 for (lo, hi) = PAIRS[c].  A row of genotype plane bits (tests/concordance_model.py) is het
at p with pair c when V and H are set and exactly two of A/C/G/T.  Only the primary record (slot r < P) of (row, p) enters:
k_lo = fw[lo] + bw[lo], k_hi likewise, m = k_lo + k_hi.

The binomial tail shares nothing with csrc/ampli_math.h: the first term comes from lgamma (m <= LGAMMA_MAX_M, where its rounding error
is below 1e-8 of the term) or from mpmath at 50 digits (deeper), the later ones from the exact ratio, summed until a term is below
1e-16 of the sum."""
import functools
import math

import numpy as np

ABSENT = np.iinfo(np.int32).min
PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
NOT_HET, ABSENT_REC, SHALLOW, DEEP, NO_REFERENCE, TESTED_REF, TESTED_HALF = range(7)
STATUS = ("NOT_HET", "ABSENT", "SHALLOW", "DEEP", "NO_REFERENCE", "TESTED_REF", "TESTED_HALF")
NO_PAIR = 7
NA = np.float32(-999.0)
MAX_M = 2 ** 31 - 1
SITES, SIG, DEPTH, DEV16, Q20 = range(5)
FEW, BALANCED, IMBALANCED = 0, 1, 2
VERDICT = ("FEW", "BALANCED", "IMBALANCED")
DEFAULTS = dict(min_depth=100, min_normals=5, site_q=20.0, min_sites=3, q_min=20.0, min_imbalance=0.02)
LGAMMA_MAX_M = 1 << 20
P2_ONE = 1.0 - 1e-8  # a two-sided p within 1e-8 of 1 is 1: the kernels' sums end 1e-9 short of their tails, and 2 p = 1 exactly is common (m odd, v = 0.5)
_BITS_TO_PAIR = {3: 0, 5: 1, 9: 2, 6: 3, 10: 4, 12: 5}


# ---- het sites ---------------------------------------------------------------------------------------------------------------------------

def pair_codes(bits):
    """uint8 [...] plane bits (V, A, C, G, T, H = bits 0..5) -> int8 [...] pair code, -1 where the bits are not a het site"""
    bits = np.asarray(bits).astype(np.int64)
    table = np.full(64, -1, np.int8)
    for g in range(64):
        if (g & 1) and (g & 32):
            table[g] = _BITS_TO_PAIR.get((g >> 1) & 15, -1)
    return table[bits & 63]


def unpack_planes(planes, P):
    """uint64 [n, 6, W] -> uint8 [n, P] plane bits"""
    planes = np.asarray(planes).view(np.uint64)
    n, _, W = planes.shape
    out = np.zeros((n, W * 64), np.uint8)
    shift = np.arange(64, dtype=np.uint64)
    for k in range(6):
        out |= (((planes[:, k, :, None] >> shift) & np.uint64(1)).reshape(n, W * 64).astype(np.uint8) << k).astype(np.uint8)
    return out[:, :P]


def pair_reads(recs, P, codes):
    """int32 [n, >= P, 8] records and int8 [n, P] pair codes -> present bool, k_lo, k_hi int64 [n, P] (0 where there is no pair)"""
    r = np.asarray(recs)[:, :P].astype(np.int64)
    present = r[..., 0] != ABSENT
    tot = r[..., :4] + r[..., 4:]
    lo = np.array([p[0] for p in PAIRS] + [0])[codes]
    hi = np.array([p[1] for p in PAIRS] + [0])[codes]
    k_lo = np.take_along_axis(tot, lo[..., None], -1)[..., 0]
    k_hi = np.take_along_axis(tot, hi[..., None], -1)[..., 0]
    ok = present & (codes >= 0)
    return present, np.where(ok, k_lo, 0), np.where(ok, k_hi, 0)


# ---- stage R -----------------------------------------------------------------------------------------------------------------------------

def reference(recs, bits, P, min_depth, ref=None):
    """the chunk's rows added to ref int64 [3, 6, P] (CNT, LO, HI); bits: the plane bits of the chunk's own rows, uint8 [n, P]"""
    ref = np.zeros((3, 6, P), np.int64) if ref is None else np.array(ref, np.int64)
    codes = pair_codes(np.asarray(bits)[:, :P])
    present, k_lo, k_hi = pair_reads(recs, P, codes)
    take = (codes >= 0) & present & (k_lo + k_hi >= min_depth)
    for c in range(6):
        t = take & (codes == c)
        ref[0, c] += t.sum(0)
        ref[1, c] += np.where(t, k_lo, 0).sum(0)
        ref[2, c] += np.where(t, k_hi, 0).sum(0)
    return ref


# ---- the tail ----------------------------------------------------------------------------------------------------------------------------

_lgamma = np.frompyfunc(math.lgamma, 1, 1)


def _first_terms(n, j, w):
    """pmf(j) of Bin(n, w) for float64 arrays, n <= LGAMMA_MAX_M"""
    lg = lambda x: _lgamma(x + 1.0).astype(np.float64)
    return np.exp(lg(n) - lg(j) - lg(n - j) + j * np.log(w) + (n - j) * np.log1p(-w))


@functools.lru_cache(maxsize=1 << 14)
def _tail_deep(n, j, w):
    """P[X >= j], X ~ Bin(n, w), at 50 digits: for the reads beyond LGAMMA_MAX_M"""
    from mpmath import mp

    from fractions import Fraction

    with mp.workdps(50):
        W = mp.mpf(w)
        lf = lambda x: mp.loggamma(x + 1)
        first = mp.exp(lf(n) - lf(j) - lf(n - j) + j * mp.log(W) + (n - j) * mp.log1p(-W))
    odds = Fraction(w) / (1 - Fraction(w))  # a float64 is a rational: the ratios are exact integers over integers
    num, den = odds.numerator, odds.denominator
    t = s = 1 << 160  # the terms relative to the first one, in 160-bit fixed point
    x = j
    while x < n and t > (s >> 70):
        t = t * ((n - x) * num) // ((x + 1) * den)
        s += t
        x += 1
    with mp.workdps(50):
        return float(first * mp.mpf(s) / mp.mpf(1 << 160))


def upper_tails(n, j, w):
    """P[X >= j], X ~ Bin(n, w), for arrays of integers n, j (n w < j <= n) and float64 w in (0, 1)"""
    n, j, w = np.asarray(n, np.int64), np.asarray(j, np.int64), np.asarray(w, np.float64)
    out = np.zeros(n.shape, np.float64)
    deep = n > LGAMMA_MAX_M
    for i in np.flatnonzero(deep):
        out[i] = _tail_deep(int(n[i]), int(j[i]), float(w[i]))
    idx = np.flatnonzero(~deep)
    if len(idx):
        nn, x, ww = n[idx].astype(np.float64), j[idx].astype(np.float64), w[idx]
        o = ww / (1.0 - ww)
        t = _first_terms(nn, x, ww)
        s = t.copy()
        live = np.ones(len(idx), bool)
        while live.any():
            r = (nn - x) / (x + 1.0) * o
            t = np.where(live, t * r, t)
            s = np.where(live, s + t, s)
            x = x + 1.0
            live &= (t > 1e-16 * s) & (x <= nn)
        out[idx] = s
    return np.minimum(out, 1.0)


def site_scores(k_lo, m, v):
    """float32 q and float64 (unrounded) of tested cells: int64 arrays k_lo, m (1 <= m <= MAX_M) and float64 v in (0, 1)"""
    k_lo, m, v = np.asarray(k_lo, np.int64), np.asarray(m, np.int64), np.asarray(v, np.float64)
    e = v * m.astype(np.float64)
    d = k_lo.astype(np.float64) - e
    up, dn = d > 0, d < 0
    p = np.ones(k_lo.shape, np.float64)
    if up.any():
        p[up] = upper_tails(m[up], k_lo[up], v[up])
    if dn.any():
        p[dn] = upper_tails(m[dn], (m - k_lo)[dn], 1.0 - v[dn])
    p2 = np.minimum(1.0, 2.0 * p)
    q64 = np.where(d == 0, 0.0, -10.0 * np.log10(np.maximum(p2, 1e-10)))
    q64 = np.where(p2 >= P2_ONE, 0.0, q64)
    q = q64.astype(np.float32)
    sign = np.where(dn & (q != 0), -1.0, 1.0)
    return (q * sign.astype(np.float32)) + np.float32(0.0), q64 * sign + 0.0


# ---- stage S -----------------------------------------------------------------------------------------------------------------------------

def cell_status(codes, present, k_lo, k_hi, cnt, lo, hi, min_depth, min_normals, half_fallback):
    """status uint8 and v float64 of cells given apart (arrays of one shape)"""
    m = k_lo + k_hi
    has_ref = (cnt >= min_normals) & (lo > 0) & (hi > 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        share = lo.astype(np.float64) / (lo + hi).astype(np.float64)
    status = np.full(codes.shape, NO_REFERENCE, np.uint8)
    v = np.zeros(codes.shape, np.float64)
    if half_fallback:
        status[:] = TESTED_HALF
        v[:] = 0.5
    status = np.where(has_ref, TESTED_REF, status)
    v = np.where(has_ref, share, v)
    for st, cond in ((DEEP, m > MAX_M), (SHALLOW, m < min_depth), (ABSENT_REC, ~present), (NOT_HET, codes < 0)):
        status = np.where(cond, st, status)
    v = np.where(status >= TESTED_REF, v, 0.0)
    return status.astype(np.uint8), v


def sites(recs, P, bits_g, row_g, ref, min_depth=100, min_normals=5, half_fallback=True):
    """recs int32 [n, >= P, 8]; bits_g uint8 [n_g, P] plane bits; row_g [n] (outside [0, n_g): none); ref int64 [3, 6, P]
    -> q float32 [n, P], km int32 [n, P, 2], v float64 [n, P], code uint8 [n, P], q64 float64 [n, P] (the unrounded score)"""
    recs, bits_g, ref = np.asarray(recs), np.asarray(bits_g), np.asarray(ref, np.int64)
    n, n_g = recs.shape[0], bits_g.shape[0]
    codes = np.full((n, P), -1, np.int8)
    for s, g in enumerate(np.asarray(row_g, np.int64)):
        if 0 <= g < n_g:
            codes[s] = pair_codes(bits_g[g, :P])
    present, k_lo, k_hi = pair_reads(recs, P, codes)
    cc = np.where(codes >= 0, codes, 0).astype(np.int64)
    pp = np.broadcast_to(np.arange(P), (n, P))
    status, v = cell_status(codes, present, k_lo, k_hi, ref[0][cc, pp], ref[1][cc, pp], ref[2][cc, pp], min_depth, min_normals, half_fallback)
    tested = status >= TESTED_REF
    q = np.full((n, P), NA, np.float32)
    q64 = np.full((n, P), float(NA), np.float64)
    km = np.zeros((n, P, 2), np.int32)
    if tested.any():
        q[tested], q64[tested] = site_scores(k_lo[tested], (k_lo + k_hi)[tested], v[tested])
        km[..., 0] = np.where(tested, k_lo, 0)
        km[..., 1] = np.where(tested, k_lo + k_hi, 0)
    code = (status.astype(np.int64) * 8 + np.where(codes >= 0, codes, NO_PAIR)).astype(np.uint8)
    return q, km, v, code, q64


# ---- stage G -----------------------------------------------------------------------------------------------------------------------------

def site_sums(q, km, v):
    """DEV16 and Q20 addends of tested cells"""
    k, m = km[..., 0].astype(np.float64), km[..., 1].astype(np.float64)
    e = v * m
    dev16 = np.rint(np.abs(k - e) * 16.0).astype(np.int64)
    q20 = np.rint(np.abs(q.astype(np.float64)) * 1048576.0).astype(np.int64)
    return dev16, q20


def region_sums(q, km, v, code, reg_off, reg_pos, site_q):
    """the five sums int64 [S, R, 5] over the regions' position lists (a CSR; entries >= P are none)"""
    S, P = q.shape
    R = len(reg_off) - 1
    W = len(reg_pos)
    tested = ((code >> 3) >= TESTED_REF) & (q != NA)
    dev16, q20 = site_sums(q, km, v)
    out = np.zeros((S, R, 5), np.int64)
    for r in range(R):
        a = min(int(reg_off[r]), W)
        b = max(a, min(int(reg_off[r + 1]), W))
        pos = np.asarray(reg_pos[a:b], np.int64)
        pos = pos[pos < P]
        if not len(pos):
            continue
        t = tested[:, pos]
        out[:, r, SITES] = t.sum(1)
        out[:, r, SIG] = (t & (np.abs(q[:, pos].astype(np.float64)) >= site_q)).sum(1)
        out[:, r, DEPTH] = np.where(t, km[:, pos, 1].astype(np.int64), 0).sum(1)
        out[:, r, DEV16] = np.where(t, dev16[:, pos], 0).sum(1)
        out[:, r, Q20] = np.where(t, q20[:, pos], 0).sum(1)
    return out


# ---- the verdict -------------------------------------------------------------------------------------------------------------------------

def kf_lgamma(z):
    x = 0.0
    x += 0.1659470187408462e-06 / (z + 7)
    x += 0.9934937113930748e-05 / (z + 6)
    x -= 0.1385710331296526 / (z + 5)
    x += 12.50734324009056 / (z + 4)
    x -= 176.6150291498386 / (z + 3)
    x += 771.3234287757674 / (z + 2)
    x -= 1259.139216722289 / (z + 1)
    x += 676.5203681218835 / z
    x += 0.9999999999995183
    return math.log(x) - 5.58106146679532777 - z + (z - 0.5) * math.log(z + 6.5)


def kf_gammaq(s, z):
    """the project's kf_gammaq (csrc/ampli_math.h: samtools' kfunc.c with its 99-step caps), operation for operation"""
    if z <= 1.0 or z < s:
        total, x = 1.0, 1.0
        for k in range(1, 100):
            x *= z / (s + k)
            total += x
            if x / total < 1e-14:
                break
        lz = math.log(z) if z > 0 else -math.inf
        return 1.0 - math.exp(s * lz - z - kf_lgamma(s + 1.0) + math.log(total))
    f = 1.0 + z - s
    Cc, D = f, 0.0
    for j in range(1, 100):
        a, b = j * (s - j), (j << 1) + 1 + z - s
        D = b + a * D
        if D < 1e-290:
            D = 1e-290
        Cc = b + a / Cc
        if Cc < 1e-290:
            Cc = 1e-290
        D = 1.0 / D
        d = Cc * D
        f *= d
        if abs(d - 1.0) < 1e-14:
            break
    return math.exp(s * math.log(z) - z - kf_lgamma(s) - math.log(f))


def region_verdict(sums, min_sites=3, q_min=20.0, min_imbalance=0.02):
    """(verdict, Q, imbalance) of the five sums of one (sample, region); NaN where a figure does not exist"""
    sites_, depth = int(sums[SITES]), int(sums[DEPTH])
    imb = float(int(sums[DEV16])) / (16.0 * float(depth)) if depth > 0 else math.nan
    if sites_ < min_sites or sites_ < 1:
        return FEW, math.nan, imb
    X = (2.302585092994046 / 5.0) * (float(int(sums[Q20])) / 1048576.0)
    p = kf_gammaq(float(sites_), X / 2.0)
    Q = 0.0 if p >= 1.0 else (-10.0 * math.log10(p) if p > 1e-30 else 300.0)
    return (IMBALANCED if (Q >= q_min and imb >= min_imbalance) else BALANCED), Q, imb


def fraction_cnloh(imb):
    return 2.0 * imb


def fraction_loss(imb):
    return 4.0 * imb / (1.0 + 2.0 * imb)


def term_bound(m, v):
    return 8.0 * np.sqrt(np.asarray(m, np.float64) * v * (1.0 - v)) + 64.0


# ---- the command line's files --------------------------------------------------------------------------------------------------------------

PAIR_NAMES = ("A/C", "A/G", "A/T", "C/G", "C/T", "G/T")


def _num(fmt, x):
    return "NA" if (isinstance(x, float) and math.isnan(x)) else fmt % x


def bed_regions(rows):
    """rows [(chrom, start, end, name, rs, gene)] -> positions [(chrom, coordinate)] in order of first appearance in the walk, region
    names (the gene strings in byte order, then ALL), reg_off, reg_pos (a gene's unique positions in walk order; ALL: every position)"""
    index, positions, genes = {}, [], {}
    for chrom, start, end, _, _, gene in rows:
        g = genes.setdefault(gene, [])
        for x in range(int(start), int(end) + 1):
            p = index.setdefault((chrom, x), len(index))
            if p == len(positions):
                positions.append((chrom, x))
            if p not in g:
                g.append(p)
    names = sorted(genes, key=lambda s: s.encode())
    lists = [genes[k] for k in names] + [list(range(len(positions)))]
    off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    return positions, names + ["ALL"], off, np.concatenate([np.asarray(x, np.int64) for x in lists])


def format_files(names_n, names_2, germline_of, positions, reg_names, ref, q, km, v, code, sums, prm, with_tumours, n_pairs):
    """the four files as text.  names_n / names_2: the normals and the files of pass 2 as the Summary names samples; germline_of[s]: the
    normal's name or "self"; ref int64 [3, 6, P]; the site planes and sums of pass 2; prm: the six parameters"""
    P = len(positions)
    reference = "Chrom\tPosition\tPair\tNormals\tLo\tHi\tShare\n"
    cells = usable = 0
    for p in range(P):
        for c in range(6):
            cnt, lo, hi = int(ref[0, c, p]), int(ref[1, c, p]), int(ref[2, c, p])
            if cnt <= 0:
                continue
            cells += 1
            usable += cnt >= prm["min_normals"] and lo > 0 and hi > 0
            reference += f"{positions[p][0]}\t{positions[p][1]}\t{PAIR_NAMES[c]}\t{cnt}\t{lo}\t{hi}\t{_num('%.5f', lo / (lo + hi) if lo + hi > 0 else math.nan)}\n"
    sites_ = "Sample\tChrom\tPosition\tPair\tReference\tKlo\tM\tExpected\tObserved\tQ\n"
    tested = half = sig = 0
    for s in range(len(names_2)):
        for p in range(P):
            st = int(code[s, p]) >> 3
            if st < TESTED_REF:
                continue
            tested += 1
            half += st == TESTED_HALF
            sig += abs(float(q[s, p])) >= prm["site_q"]
            k, m = int(km[s, p, 0]), int(km[s, p, 1])
            sites_ += (f"{names_2[s]}\t{positions[p][0]}\t{positions[p][1]}\t{PAIR_NAMES[int(code[s, p]) & 7]}\t{'NORMALS' if st == TESTED_REF else 'HALF'}\t{k}\t{m}\t"
                       f"{'%.5f' % v[s, p]}\t{'%.5f' % (k / m)}\t{'%.4f' % float(q[s, p])}\n")
    genes = "Sample\tRegion\tSites\tSignificant\tDepth\tDev16\tQ20\tQ\tImbalance\tVerdict\tFractionIfCopyNeutralLOH\tFractionIfSingleCopyLoss\n"
    by = [0, 0, 0]
    for s in range(len(names_2)):
        for r, name in enumerate(reg_names):
            x = [int(t) for t in sums[s, r]]
            verdict, Q, imb = region_verdict(x, prm["min_sites"], prm["q_min"], prm["min_imbalance"])
            by[verdict] += 1
            genes += (f"{names_2[s]}\t{name}\t" + "\t".join(str(t) for t in x) + f"\t{_num('%.4f', Q)}\t{_num('%.5f', imb)}\t{VERDICT[verdict]}\t"
                      f"{_num('%.5f', imb if math.isnan(imb) else fraction_cnloh(imb))}\t{_num('%.5f', imb if math.isnan(imb) else fraction_loss(imb))}\n")
    n_t = by[BALANCED] + by[IMBALANCED]
    summary = (f"normals={len(names_n)}\nfiles={len(names_2)}\nmode={'tumours' if with_tumours else 'null_calibration'}\npairs={n_pairs}\npositions={P}\n"
               f"regions={len(reg_names)}\nmin_depth={prm['min_depth']}\nmin_normals={prm['min_normals']}\nsite_q={'%g' % prm['site_q']}\nmin_sites={prm['min_sites']}\n"
               f"q_min={'%g' % prm['q_min']}\nmin_imbalance={'%g' % prm['min_imbalance']}\nreference_cells={cells}\nreference_cells_usable={usable}\n"
               f"sites_tested={tested}\nsites_tested_half={half}\nsites_significant={sig}\nregions_few={by[FEW]}\nregions_balanced={by[BALANCED]}\n"
               f"regions_imbalanced={by[IMBALANCED]}\nshare_flagged={_num('%.5f', by[IMBALANCED] / n_t if n_t else math.nan)}\nSample\tGermline\n")
    summary += "".join(f"{n}\t{g}\n" for n, g in zip(names_2, germline_of))
    return {"Allelic_Reference.txt": reference, "Allelic_Sites.txt": sites_, "Allelic_Genes.txt": genes, "Allelic_Summary.txt": summary}
