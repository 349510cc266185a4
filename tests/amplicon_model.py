"""Amplicon coverage and copy ratio against the panel of normals -- THE DEFINITION, in plain numpy (TEST INFRASTRUCTURE; DESIGN 16, and
the comment over ampli_amplicon_depth_records in include/amplisolve_hip.h).  The kernels of ampli_amplicon.hip and the host functions of
ampli_math.h are compared with this file exactly: the integer sums with np.array_equal, the doubles bit for bit with NaNs matched by
position.

Amplicon lists: a CSR over the BED walk, amp_off [A + 1] and amp_pos [W] with entries in [0, P).  Lists may overlap and be in any
order; a position may be in several lists and more than once in one; a list may be empty.

Stage 1 (depth_sums): per (sample s, amplicon a) four int64 sums over the entries p of a's list, from the primary record (s, p) only:
PRESENT += 1 where the record is present, DEPTH_FW += FW, DEPTH_BW += BW, CALLABLE += 1 where FW >= cutoff and BW >= cutoff; FW and BW
are the sums of the four forward and the four reverse counts; an absent record adds nothing.

Stage 2a (reference), 2b (ratios) and the gene level: see the functions.  Every floating-point operation is one IEEE double operation
in the written order; numpy does not fuse, and both libraries are built with -ffp-contract=off."""
import numpy as np

ABSENT = np.iinfo(np.int32).min
PRESENT, DEPTH_FW, DEPTH_BW, CALLABLE = range(4)
OK, FEW, DARK = range(3)
NEUTRAL, GAIN, LOSS = range(3)
STATUS_NAMES = ("OK", "FEW", "DARK")
GENE_NAMES = ("NEUTRAL", "GAIN", "LOSS")
DEFAULTS = dict(coverage_cutoff=100, min_normals=5, min_amplicons=3, z_cutoff=3.0, gain_ratio=1.3, loss_ratio=0.7)


def depth_sums(recs, amp_off, amp_pos, cutoff=100):
    """recs int32 [n, >= P, 8] (only slots named by amp_pos are read) -> int64 [n, A, 4]"""
    recs = np.asarray(recs)
    amp_off, amp_pos = np.asarray(amp_off, np.int64), np.asarray(amp_pos, np.int64)
    n, A = recs.shape[0], len(amp_off) - 1
    out = np.zeros((n, A, 4), np.int64)
    for a in range(A):
        r = recs[:, amp_pos[amp_off[a]:amp_off[a + 1]], :].astype(np.int64)  # [n, len, 8]: a repeated entry is read again
        present = r[:, :, 0] != ABSENT
        fw, bw = r[:, :, :4].sum(-1), r[:, :, 4:].sum(-1)
        out[:, a, PRESENT] = present.sum(1)
        out[:, a, DEPTH_FW] = np.where(present, fw, 0).sum(1)
        out[:, a, DEPTH_BW] = np.where(present, bw, 0).sum(1)
        out[:, a, CALLABLE] = (present & (fw >= cutoff) & (bw >= cutoff)).sum(1)
    return out


def median(v):
    """THE median, used everywhere: over m doubles in ascending order, m odd v[(m-1)/2], m even (v[m/2-1] + v[m/2]) * 0.5, m == 0 NaN.
    (The kernels take finite non-negative values and select on the bit patterns; the gene level takes signed ones -- use median_nan.)"""
    v = np.sort(np.asarray(v, np.float64))
    m = len(v)
    if m == 0:
        return np.float64(np.nan)
    if m & 1:
        return v[(m - 1) // 2]
    return (v[m // 2 - 1] + v[m // 2]) * np.float64(0.5)


def median_nan(v):
    """the median of the values that are not NaN (the gene level: signed values, by ascending sort)"""
    v = np.asarray(v, np.float64)
    return median(v[~np.isnan(v)])


def totals(sums, use):
    """T[s] = the sum of DEPTH_FW + DEPTH_BW over the amplicons with use[a], in int64"""
    sums = np.asarray(sums, np.int64)
    d = sums[:, :, DEPTH_FW] + sums[:, :, DEPTH_BW]
    return d[:, np.asarray(use) != 0].sum(1)


def reference(sums, use, min_normals=5):
    """from the normals' sums int64 [N, A, 4]: dict total int64 [N], n_eff, med, mad float64 [A], status uint8 [A]"""
    sums = np.asarray(sums, np.int64)
    N, A = sums.shape[:2]
    d = sums[:, :, DEPTH_FW] + sums[:, :, DEPTH_BW]
    T = totals(sums, use)
    inc = T > 0
    n_eff = int(inc.sum())
    x = d[inc].astype(np.float64) / T[inc].astype(np.float64)[:, None]
    med, mad = np.empty(A, np.float64), np.empty(A, np.float64)
    for a in range(A):
        med[a] = median(x[:, a])
        mad[a] = median(np.abs(x[:, a] - med[a]))
    if n_eff < min_normals:
        status = np.full(A, FEW, np.uint8)
    else:
        status = np.where(med == 0, DARK, OK).astype(np.uint8)
    return dict(total=T, n_eff=n_eff, med=med, mad=mad, status=status)


def z_of(ratio, med, mad):
    with np.errstate(all="ignore"):
        num = (np.asarray(ratio, np.float64) - np.float64(1.0)) * med
        den = np.float64(1.4826) * np.asarray(mad, np.float64)
        return np.where(np.asarray(mad) > 0, num / den, np.nan)


def ratios(sums, use, ref):
    """any set of samples int64 [S, A, 4] against a reference: dict total int64 [S], centre float64 [S], k int32 [S], ratio, z [S, A].
    K[s] counts the amplicons with use[a] and status OK, and is 0 for a sample with T[s] <= 0; the centre of K == 0 values is NaN."""
    sums = np.asarray(sums, np.int64)
    S, A = sums.shape[:2]
    use = np.asarray(use) != 0
    d = sums[:, :, DEPTH_FW] + sums[:, :, DEPTH_BW]
    T = totals(sums, use)
    ok = ref["status"] == OK
    ratio, centre, k = np.full((S, A), np.nan), np.full(S, np.nan), np.zeros(S, np.int32)
    with np.errstate(all="ignore"):
        for s in range(S):
            if T[s] <= 0:
                continue
            x = d[s].astype(np.float64) / np.float64(T[s])
            r = np.where(ok, x / ref["med"], np.nan)
            sel = use & ok
            k[s] = sel.sum()
            centre[s] = median(r[sel])
            ratio[s] = r / centre[s]
    z = z_of(ratio, ref["med"][None, :], np.broadcast_to(ref["mad"][None, :], (S, A)))
    return dict(total=T, centre=centre, k=k, ratio=ratio, z=z)


def gene_status(n, median_ratio, median_z, min_amplicons=3, gain_ratio=1.3, loss_ratio=0.7, z_cutoff=3.0):
    if n >= min_amplicons and median_ratio >= gain_ratio and median_z >= z_cutoff:
        return GAIN
    if n >= min_amplicons and median_ratio <= loss_ratio and median_z <= -z_cutoff:
        return LOSS
    return NEUTRAL


def genes(ratio, z, status, gene_of, **kw):
    """per (sample, gene string), over the gene's OK amplicons: {(s, gene): (n, median ratio, median z, status)}; the medians drop NaNs"""
    out = {}
    names = sorted(set(gene_of))
    gene_of = np.asarray(gene_of)
    for s in range(ratio.shape[0]):
        for g in names:
            sel = (gene_of == g) & (status == OK)
            n = int(sel.sum())
            mr, mz = median_nan(ratio[s, sel]), median_nan(z[s, sel])
            out[s, g] = (n, mr, mz, gene_status(n, mr, mz, **kw))
    return out


def same(a, b):
    """np.array_equal with NaNs matched by position, bit for bit elsewhere (and -0.0 is not 0.0)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(np.int64), b[~nb].view(np.int64)))


# ---- the command line: the lists of a BED and the bytes of the four files ----

def read_bed(text):
    """rows (chrom, start, end, name, gene) as the host reads them: whitespace-separated, name column 4 and gene column 6, '.' where
    the row has no such column"""
    rows = []
    for line in text.splitlines():
        f = line.split()
        if f:
            rows.append((f[0], int(f[1]), int(f[2]), f[3] if len(f) > 3 else ".", f[5] if len(f) > 5 else "."))
    return rows


def bed_lists(rows, exclude=("chrX", "chrY")):
    """the position index and the amplicons' lists of a BED: positions are numbered in the order the walk first meets them; amplicon a's
    list is its walk entries whose position is listed once in the whole BED, or all its entries if that leaves none; use[a] = 0 on the
    excluded chromosomes.  Returns P, walk, dup, amp_off, amp_pos, use."""
    index, walk, dup = {}, [], []
    for c, a, b, _, _ in rows:
        for x in range(a, b + 1):
            if (c, x) in index:
                dup[index[c, x]] = 1
            else:
                index[c, x] = len(index)
                dup.append(0)
            walk.append(index[c, x])
    off, pos, w = [0], [], 0
    for c, a, b, _, _ in rows:
        mine = walk[w:w + max(0, b - a + 1)]
        w += len(mine)
        pos += [p for p in mine if not dup[p]] or mine
        off.append(len(pos))
    use = np.array([0 if c in exclude else 1 for c, *_ in rows], np.uint8)
    return len(index), np.array(walk, np.uint32), np.array(dup, np.uint8), np.array(off, np.uint32), np.array(pos, np.uint32), use


def _num(fmt, x):
    return "NA" if x != x else fmt % x


def format_files(names, n_normals, rows, amp_off, sums, ref, rat, exclude_chrom="chrX,chrY", with_tumours=True, coverage_cutoff=100, min_normals=5,
                 min_amplicons=3, z_cutoff=3.0, gain_ratio=1.3, loss_ratio=0.7):
    """the bytes of Amplicon_Reference.txt, Amplicon_Ratios.txt, Amplicon_Genes.txt and Amplicon_Summary.txt: shares '%.6e', ratios
    and centres '%.5f', z '%.3f', callable fractions '%.4f', parameters '%g', NaN as NA"""
    S, A = sums.shape[:2]
    length = np.diff(np.asarray(amp_off, np.int64))
    sets = ["N" if s < n_normals else "T" for s in range(S)]
    out = {}
    text = "Chrom\tStart\tEnd\tAmplicon\tGene\tPositions\tStatus\tNeff\tMedian\tMAD\tCallable\n"
    for a, (c, lo, hi, name, gene) in enumerate(rows):
        callable_ = int(sums[:n_normals, a, CALLABLE].sum())
        fraction = np.float64(callable_) / np.float64(n_normals * int(length[a])) if length[a] > 0 else np.nan
        text += (f"{c}\t{lo}\t{hi}\t{name}\t{gene}\t{length[a]}\t{STATUS_NAMES[ref['status'][a]]}\t{ref['n_eff']}\t{_num('%.6e', ref['med'][a])}\t"
                 f"{_num('%.6e', ref['mad'][a])}\t{_num('%.4f', fraction)}\n")
    out["Amplicon_Reference.txt"] = text
    text = "Sample\tSet\tAmplicon\tGene\tPresent\tDepthFw\tDepthBw\tCallable\tRatio\tZ\n"
    for s in range(S):
        for a, (_, _, _, name, gene) in enumerate(rows):
            c = sums[s, a]
            text += f"{names[s]}\t{sets[s]}\t{name}\t{gene}\t{c[0]}\t{c[1]}\t{c[2]}\t{c[3]}\t{_num('%.5f', rat['ratio'][s, a])}\t{_num('%.3f', rat['z'][s, a])}\n"
    out["Amplicon_Ratios.txt"] = text
    g = genes(rat["ratio"], rat["z"], ref["status"], [r[4] for r in rows], min_amplicons=min_amplicons, gain_ratio=gain_ratio, loss_ratio=loss_ratio,
              z_cutoff=z_cutoff)
    text = "Sample\tSet\tGene\tAmplicons\tMedianRatio\tMedianZ\tStatus\n"
    gains = losses = 0
    for s in range(n_normals if with_tumours else 0, S):
        for gene in sorted({r[4] for r in rows}, key=lambda x: x.encode()):
            n, mr, mz, st = g[s, gene]
            gains += st == GAIN
            losses += st == LOSS
            if with_tumours and st == NEUTRAL:
                continue
            text += f"{names[s]}\t{sets[s]}\t{gene}\t{n}\t{_num('%.5f', mr)}\t{_num('%.3f', mz)}\t{GENE_NAMES[st]}\n"
    out["Amplicon_Genes.txt"] = text
    st = ref["status"]
    text = (f"normals={n_normals}\ntumours={S - n_normals}\namplicons={A}\ncoverage_cutoff={coverage_cutoff}\nmin_normals={min_normals}\n"
            f"min_amplicons={min_amplicons}\nz_cutoff={'%g' % z_cutoff}\ngain_ratio={'%g' % gain_ratio}\nloss_ratio={'%g' % loss_ratio}\n"
            f"exclude_chrom={exclude_chrom}\nn_eff={ref['n_eff']}\namplicons_ok={(st == OK).sum()}\namplicons_few={(st == FEW).sum()}\n"
            f"amplicons_dark={(st == DARK).sum()}\ngenes_gain={gains}\ngenes_loss={losses}\n")
    text += "Sample\tSet\tTotal\tCentre\tK\tBelowCallable\n"
    for s in range(S):
        below = int((sums[s, :, CALLABLE] < length).sum())
        text += f"{names[s]}\t{sets[s]}\t{rat['total'][s]}\t{_num('%.5f', rat['centre'][s])}\t{rat['k'][s]}\t{below}\n"
    out["Amplicon_Summary.txt"] = text
    return out
