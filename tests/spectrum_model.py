"""Substitution spectrum and strand asymmetry -- THE DEFINITION, in plain numpy (TEST INFRASTRUCTURE; DESIGN 17, and the comment over
ampli_spectrum_records in include/amplisolve_hip.h).  spectrum_kernel and the host functions of ampli_math.h are compared with this file
exactly: the integer sums with np.array_equal, the doubles bit for bit with NaNs matched by position.

Stage 1 (class_sums): per (sample s, class c) nine int64 sums over the positions p with cls[p] == c whose PRIMARY record (s, p) enters:
SITES += 1, FW_A..FW_T += fw[b], BW_A..BW_T += bw[b].  The record enters iff it is present, ref_code[p] is 0..3, cls[p] < C, FW >= cutoff
and BW >= cutoff, and 1000 n_b <= max_alt_pm d for every base b other than the reference (n_b = fw[b] + bw[b], d = FW + BW): the
position is background for this file.  d == 0 passes the last clause and is stopped only by a positive cut-off.

Stage 2 (fold, score): see the functions.  Every floating-point operation is one IEEE double operation in the written order; numpy
does not fuse, and the host library is built with -ffp-contract=off."""
import numpy as np

from tests.amplicon_model import median_nan, same  # noqa: F401  (same: re-exported for the tests)

ABSENT = np.iinfo(np.int32).min
SITES, FW_A, FW_C, FW_G, FW_T, BW_A, BW_C, BW_G, BW_T = range(9)
SUMS, MAX_CLASSES, CLASSES, SKIP, TYPES, ALL, CHANNELS = 9, 128, 68, 255, 13, 12, 96
OK, LOW_SITES, NO_REFERENCE, ELEVATED, ASYMMETRIC = range(5)
REF_OK, REF_FEW = range(2)
FLAG_NAMES = ("OK", "LOW_SITES", "NO_REFERENCE", "ELEVATED", "ASYMMETRIC")
REF_NAMES = ("OK", "FEW")
NT = "ACGT"
TYPE_NAMES = tuple(f"{NT[r]}>{NT[y]}" for r in range(4) for y in range(4) if y != r) + ("ALL",)
DEFAULTS = dict(coverage_cutoff=100, max_alt_pm=30, min_sites=200, min_normals=5, excess_ratio=3.0, z_cutoff=10.0, asym_delta=0.15)


# ---- stage 1 ----

def enters(recs, ref_code, cls, C, cutoff=100, max_alt_pm=30):
    """recs int32 [..., 8], ref_code and cls uint8 broadcast against recs[..., 0] -> bool [...]"""
    r = np.asarray(recs).astype(np.int64)
    ref, cls = np.asarray(ref_code).astype(np.int64), np.asarray(cls).astype(np.int64)
    present = r[..., 0] != ABSENT
    n = r[..., :4] + r[..., 4:]
    FW, BW = r[..., :4].sum(-1), r[..., 4:].sum(-1)
    lim = max_alt_pm * (FW + BW)
    other = np.arange(4) != ref[..., None]
    background = (~other | (1000 * n <= lim[..., None])).all(-1)
    return present & (ref >= 0) & (ref <= 3) & (cls < C) & (FW >= cutoff) & (BW >= cutoff) & background


def class_sums(recs, ref_code, cls, C, cutoff=100, max_alt_pm=30):
    """recs int32 [n, >= P, 8] (only the slots below P = len(cls) are read) -> int64 [n, C, 9]"""
    cls = np.asarray(cls)
    P = len(cls)
    r = np.asarray(recs)[:, :P].astype(np.int64)
    e = enters(recs[:, :P], np.asarray(ref_code)[None, :], cls[None, :], C, cutoff, max_alt_pm)
    vals = np.concatenate([np.ones(r.shape[:2] + (1,), np.int64), r], axis=-1) * e[..., None]
    out = np.zeros((r.shape[0], C, SUMS), np.int64)
    for c in np.unique(cls[cls < C]):
        out[:, c] = vals[:, cls == c].sum(1)
    return out


# ---- the command line's classes ----

def base_code(s):
    """the code of a reference-base string as a neighbour sees it: upper-cased, one of A C G T, else 255"""
    s = s.upper() if len(s) == 1 and "a" <= s <= "z" else s
    return NT.index(s) if len(s) == 1 and s in NT else 255


def spectrum_class(r, l, t):
    if r > 3:
        return SKIP
    return 16 * r + 4 * l + t if l <= 3 and t <= 3 else 64 + r


def panel_classes(positions, bases):
    """positions: [(chrom, coordinate)] of the panel; bases: {(chrom, coordinate): reference-base string}, the panel's own.  The
    reference code is the exact, case-sensitive match of the host (a lower-case base is not a reference base); the neighbours are
    upper-cased.  Returns ref_code, cls uint8 [P]."""
    have = set(positions)
    ref = np.array([NT.index(bases.get(p, "")) if bases.get(p, "") in tuple(NT) else 255 for p in positions], np.uint8)

    def code(c, x):
        return base_code(bases.get((c, x), "")) if (c, x) in have else 255

    cls = np.array([spectrum_class(int(r), code(c, x - 1), code(c, x + 1)) for r, (c, x) in zip(ref, positions)], np.uint8)
    return ref, cls


# ---- stage 2 ----

def alt_index(r, y):
    return y if y < r else y - 1


def channel_of(c, y):
    """the channel (0..95) of alternative y in class c < 64"""
    r, l, t = c >> 4, (c >> 2) & 3, c & 3
    if r in (0, 2):
        r, l, t, y = 3 - r, 3 - t, 3 - l, 3 - y
    return 16 * ((3 if r == 3 else 0) + alt_index(r, y)) + 4 * l + t


def channel_name(ch):
    sub, l, t = ch // 16, (ch // 4) % 4, ch % 4
    r = 3 if sub >= 3 else 1
    y = [b for b in range(4) if b != r][sub % 3]
    return f"{NT[l]}[{NT[r]}>{NT[y]}]{NT[t]}"


def fold(sums):
    """int64 [S, 68, 9] -> dict alt, dep int64 [S, 2, 13], sites int64 [S, 13], ctx_alt, ctx_dep int64 [S, 96]"""
    sums = np.asarray(sums, np.int64)
    S = sums.shape[0]
    assert sums.shape[1:] == (CLASSES, SUMS)
    alt, dep, sites = np.zeros((S, 2, TYPES), np.int64), np.zeros((S, 2, TYPES), np.int64), np.zeros((S, TYPES), np.int64)
    ctx_alt, ctx_dep = np.zeros((S, CHANNELS), np.int64), np.zeros((S, CHANNELS), np.int64)
    for c in range(CLASSES):
        r = c >> 4 if c < 64 else c - 64
        count = sums[:, c, 1:].reshape(S, 2, 4)
        depth = count.sum(-1)
        dep[:, :, 3 * r:3 * r + 3] += depth[:, :, None]
        dep[:, :, ALL] += depth
        sites[:, 3 * r:3 * r + 3] += sums[:, c, SITES, None]
        sites[:, ALL] += sums[:, c, SITES]
        for y in range(4):
            if y == r:
                continue
            alt[:, :, 3 * r + alt_index(r, y)] += count[:, :, y]
            alt[:, :, ALL] += count[:, :, y]
            if c < 64:
                ctx_alt[:, channel_of(c, y)] += count[:, :, y].sum(1)
                ctx_dep[:, channel_of(c, y)] += depth.sum(1)
    return dict(alt=alt, dep=dep, sites=sites, ctx_alt=ctx_alt, ctx_dep=ctx_dep)


def _div(a, b, ok):
    with np.errstate(all="ignore"):
        return np.where(ok, np.asarray(a, np.float64) / np.asarray(b, np.float64), np.nan)


def rates(alt, dep):
    """alt, dep int64 [..., 2, 13] -> rate [..., 2, 13], rate2, asym [..., 13]"""
    rate = _div(alt, dep, dep > 0)
    d2 = dep[..., 0, :] + dep[..., 1, :]
    rate2 = _div(alt[..., 0, :] + alt[..., 1, :], d2, d2 > 0)
    with np.errstate(all="ignore"):
        both = rate[..., 0, :] + rate[..., 1, :]
    return rate, rate2, _div(rate[..., 0, :], both, both > 0)


def z_of(x, med, mad):
    with np.errstate(all="ignore"):
        return np.where(np.asarray(mad) > 0, (np.asarray(x, np.float64) - med) / (np.float64(1.4826) * np.asarray(mad, np.float64)), np.nan)


def flag_of(sites, few, ratio, z, asym, med_a, za, min_sites=200, excess_ratio=3.0, z_cutoff=10.0, asym_delta=0.15):
    if sites < min_sites:
        return LOW_SITES
    if few:
        return NO_REFERENCE
    if ratio >= excess_ratio and z >= z_cutoff:
        return ELEVATED
    if abs(za) >= z_cutoff and abs(asym - med_a) >= asym_delta:
        return ASYMMETRIC
    return OK


def score(f, n_normals, min_sites=200, min_normals=5, excess_ratio=3.0, z_cutoff=10.0, asym_delta=0.15):
    """the folds of S samples, the first n_normals of them the normals -> dict ref float64 [13, 4] (med, mad, med_a, mad_a), n_eff
    int32 [13], status uint8 [13], rate2, ratio, z, asym, za float64 [S, 13], flag uint8 [S, 13]"""
    alt, dep, sites = f["alt"], f["dep"], f["sites"]
    S = alt.shape[0]
    _, rate2, asym = rates(alt, dep)
    ref, n_eff, status = np.empty((TYPES, 4)), np.zeros(TYPES, np.int32), np.zeros(TYPES, np.uint8)
    ratio, z, za, flag = np.empty((S, TYPES)), np.empty((S, TYPES)), np.empty((S, TYPES)), np.zeros((S, TYPES), np.uint8)
    for ty in range(TYPES):
        inc = sites[:n_normals, ty] >= min_sites
        n_eff[ty] = inc.sum()
        status[ty] = REF_FEW if n_eff[ty] < min_normals else REF_OK
        for k, x in enumerate((rate2[:n_normals, ty][inc], asym[:n_normals, ty][inc])):
            ref[ty, 2 * k] = median_nan(x)
            ref[ty, 2 * k + 1] = median_nan(np.abs(x - ref[ty, 2 * k]))
        med, mad, med_a, mad_a = ref[ty]
        ratio[:, ty] = _div(rate2[:, ty], med, med > 0)
        z[:, ty] = z_of(rate2[:, ty], med, mad)
        za[:, ty] = z_of(asym[:, ty], med_a, mad_a)
        for s in range(S):
            flag[s, ty] = flag_of(sites[s, ty], status[ty] == REF_FEW, ratio[s, ty], z[s, ty], asym[s, ty], med_a, za[s, ty], min_sites, excess_ratio,
                                  z_cutoff, asym_delta)
    return dict(ref=ref, n_eff=n_eff, status=status, rate2=rate2, ratio=ratio, z=z, asym=asym, za=za, flag=flag)


# ---- the command line: the bytes of the four files ----

def _num(fmt, x):
    return "NA" if x != x else fmt % x


def format_files(names, n_normals, cls, sums, f, sc, coverage_cutoff=100, max_alt_pm=30, min_sites=200, min_normals=5, excess_ratio=3.0, z_cutoff=10.0,
                 asym_delta=0.15):
    """the bytes of Spectrum_Reference.txt, Spectrum_Samples.txt, Spectrum_Contexts.txt and Spectrum_Summary.txt: rates '%.6e', ratios
    and asymmetries '%.5f', z '%.3f', parameters '%g', NaN as NA"""
    S = sums.shape[0]
    sets = ["N" if s < n_normals else "T" for s in range(S)]
    out = {}
    text = "Type\tNeff\tMedian\tMAD\tMedianAsym\tMADAsym\tStatus\n"
    for ty in range(TYPES):
        med, mad, med_a, mad_a = sc["ref"][ty]
        text += (f"{TYPE_NAMES[ty]}\t{sc['n_eff'][ty]}\t{_num('%.6e', med)}\t{_num('%.6e', mad)}\t{_num('%.5f', med_a)}\t{_num('%.5f', mad_a)}\t"
                 f"{REF_NAMES[sc['status'][ty]]}\n")
    out["Spectrum_Reference.txt"] = text
    text = "Sample\tSet\tType\tSites\tAltFw\tDepthFw\tAltBw\tDepthBw\tRate\tRatio\tZ\tAsym\tZAsym\tFlag\n"
    for s in range(S):
        for ty in range(TYPES):
            a, d = f["alt"][s, :, ty], f["dep"][s, :, ty]
            text += (f"{names[s]}\t{sets[s]}\t{TYPE_NAMES[ty]}\t{f['sites'][s, ty]}\t{a[0]}\t{d[0]}\t{a[1]}\t{d[1]}\t{_num('%.6e', sc['rate2'][s, ty])}\t"
                     f"{_num('%.5f', sc['ratio'][s, ty])}\t{_num('%.3f', sc['z'][s, ty])}\t{_num('%.5f', sc['asym'][s, ty])}\t"
                     f"{_num('%.3f', sc['za'][s, ty])}\t{FLAG_NAMES[sc['flag'][s, ty]]}\n")
    out["Spectrum_Samples.txt"] = text
    text = "Sample\tSet\tChannel\tAlt\tDepth\tRate\n"
    rate = _div(f["ctx_alt"], f["ctx_dep"], f["ctx_dep"] > 0)
    for s in range(S):
        for ch in range(CHANNELS):
            text += f"{names[s]}\t{sets[s]}\t{channel_name(ch)}\t{f['ctx_alt'][s, ch]}\t{f['ctx_dep'][s, ch]}\t{_num('%.6e', rate[s, ch])}\n"
    out["Spectrum_Contexts.txt"] = text
    cls = np.asarray(cls)
    text = (f"normals={n_normals}\ntumours={S - n_normals}\npositions={len(cls)}\ncoverage_cutoff={coverage_cutoff}\nmax_alt_pm={max_alt_pm}\n"
            f"min_sites={min_sites}\nmin_normals={min_normals}\nexcess_ratio={'%g' % excess_ratio}\nz_cutoff={'%g' % z_cutoff}\n"
            f"asym_delta={'%g' % asym_delta}\npositions_trinucleotide={(cls < 64).sum()}\npositions_edge={((cls >= 64) & (cls < CLASSES)).sum()}\n"
            f"positions_skipped={(cls >= CLASSES).sum()}\nclasses_used={len(np.unique(cls[cls < CLASSES]))}\n")
    text += "Sample\tSet\tSitesA\tSitesC\tSitesG\tSitesT\tNotOK\n"
    for s in range(S):
        bad = [f"{TYPE_NAMES[ty]}:{FLAG_NAMES[sc['flag'][s, ty]]}" for ty in range(TYPES) if sc["flag"][s, ty] != OK]
        st = f["sites"][s]
        text += f"{names[s]}\t{sets[s]}\t{st[0]}\t{st[3]}\t{st[6]}\t{st[9]}\t{','.join(bad) or '-'}\n"
    out["Spectrum_Summary.txt"] = text
    return out
