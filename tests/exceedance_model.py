"""Panel-of-normals exceedance -- THE DEFINITION, in plain numpy (TEST INFRASTRUCTURE; DESIGN 18, and the comment over
ampli_exceedance_records in include/amplisolve_hip.h).  exceedance_kernel and ampli_exceedance_candidate (ampli_math.h) are compared with
this file exactly, np.array_equal on unsigned 16-bit counts and on 0 / 1.  Everything is unsigned 64-bit integer arithmetic.

Device stage (exceedance).  Only the primary record of (row, position) enters.  For strand st (0 forward, 1 reverse) x[st][b] is the count
of base b and D[st] the sum of the strand's four counts.  Normal s is ELIGIBLE for tumour t at p iff its record is present, D_s[0] >=
normal_cutoff and D_s[1] >= normal_cutoff, and not (skip_same_index and first_n + s == first_t + t).  It REACHES t at (p, b, st) iff it
is eligible and x_s[st][b] D_t[st] >= x_t[st][b] D_s[st].  elig[t][p] counts the eligible normals whatever t's own record is;
ge[t][p][b][st] counts the reaching ones where the cell is EVALUATED -- t's record present, D_t[0] >= calling_cutoff and D_t[1] >=
calling_cutoff, ref_code[p] in 0..3, b != ref_code[p] -- and is NA = 0xFFFF everywhere else.  Given the outputs of earlier chunks of
normals, this chunk's counts are added onto elig and onto the evaluated cells (modulo 2^16), and the others are NA.

Host stage (candidates): a cell (t, p, b) is a candidate iff it is evaluated, x_t[0][b] >= min_alt_reads and x_t[1][b] >= min_alt_reads,
1000 (x_t[0][b] + x_t[1][b]) >= min_vaf_pm (D_t[0] + D_t[1]), elig >= min_normals, ge[0] <= max_normals and ge[1] <= max_normals."""
import numpy as np

ABSENT = np.iinfo(np.int32).min
NA = 0xFFFF
MAX_NORMALS = 65534
NT = "ACGT"
DEFAULTS = dict(coverage_cutoff=100, calling_cutoff=100, min_alt_reads=3, min_vaf_pm=0, min_normals=10, max_normals=0)


def counts(recs):
    """int32 [..., 8] -> present bool [...], x uint64 [..., 2, 4], D uint64 [..., 2]; an absent record has no counts"""
    r = np.asarray(recs)
    present = r[..., 0] != ABSENT
    x = np.where(present[..., None], r, 0).astype(np.uint64).reshape(r.shape[:-1] + (2, 4))
    return present, x, x.sum(-1, dtype=np.uint64)


def evaluated(recs_t, ref_code, calling_cutoff=100):
    """bool [n_t, P, 4]: the cells of ge that hold a count"""
    ref_code = np.asarray(ref_code)
    P = len(ref_code)
    present, _, D = counts(np.asarray(recs_t)[:, :P])
    row = present & (D[..., 0] >= np.uint64(calling_cutoff)) & (D[..., 1] >= np.uint64(calling_cutoff)) & (ref_code <= 3)[None, :]
    return row[..., None] & (np.arange(4)[None, None, :] != ref_code[None, :, None])


def exceedance(recs_t, recs_n, ref_code, normal_cutoff=100, calling_cutoff=100, first_t=0, first_n=0, skip_same_index=False, elig=None, ge=None):
    """recs_t int32 [n_t, >= P, 8], recs_n int32 [n_n, >= P, 8] (only the slots below P = len(ref_code) are read) -> elig uint16 [n_t, P],
    ge uint16 [n_t, P, 4, 2].  elig, ge given: the accumulate form, onto copies of them."""
    ref_code = np.asarray(ref_code)
    P = len(ref_code)
    recs_t, recs_n = np.asarray(recs_t)[:, :P], np.asarray(recs_n)[:, :P]
    n_t, n_n = recs_t.shape[0], recs_n.shape[0]
    assert first_n + n_n <= MAX_NORMALS
    _, xt, Dt = counts(recs_t)
    pn, xn, Dn = counts(recs_n)
    covered = pn & (Dn[..., 0] >= np.uint64(normal_cutoff)) & (Dn[..., 1] >= np.uint64(normal_cutoff))  # [n_n, P]
    e = np.zeros((n_t, P), np.uint64)
    g = np.zeros((n_t, P, 2, 4), np.uint64)
    rows = first_t + np.arange(n_t)
    for s in range(n_n):
        ok = covered[s][None, :] & ~(skip_same_index & (rows == first_n + s))[:, None]  # [n_t, P]
        reach = xn[s][None] * Dt[..., None] >= xt * Dn[s][None, :, :, None]              # [n_t, P, 2, 4]
        e += ok
        g += reach & ok[:, :, None, None]
    g = g.transpose(0, 1, 3, 2)  # [n_t, P, 4, 2]
    ev = evaluated(recs_t, ref_code, calling_cutoff)
    if elig is not None:
        e = e + np.asarray(elig).astype(np.uint64)
        g = g + np.asarray(ge).astype(np.uint64)
    return (e & np.uint64(0xFFFF)).astype(np.uint16), np.where(ev[..., None], g & np.uint64(0xFFFF), NA).astype(np.uint16)


def candidate_cells(x, depth, elig, ge, min_alt_reads=3, min_vaf_pm=0, min_normals=10, max_normals=0):
    """x, depth uint64 [..., 2] (forward, reverse), elig uint16 [...], ge uint16 [..., 2] -> bool [...]"""
    x, depth, ge = np.asarray(x, np.uint64), np.asarray(depth, np.uint64), np.asarray(ge).astype(np.int64)
    ev = (ge[..., 0] != NA) & (ge[..., 1] != NA)
    reads = (x[..., 0] >= np.uint64(min_alt_reads)) & (x[..., 1] >= np.uint64(min_alt_reads))
    vaf = np.uint64(1000) * (x[..., 0] + x[..., 1]) >= np.uint64(min_vaf_pm) * (depth[..., 0] + depth[..., 1])
    return ev & reads & vaf & (np.asarray(elig).astype(np.int64) >= min_normals) & (ge[..., 0] <= max_normals) & (ge[..., 1] <= max_normals)


def format_files(names, n_normals, n_tumours, positions, bases, ref_code, recs, elig, ge, coverage_cutoff=100, calling_cutoff=100, min_alt_reads=3,
                 min_vaf_pm=0, min_normals=10, max_normals=0, skip_same_index=False):
    """the bytes of Exceedance_Candidates.txt, Exceedance_Samples.txt, Exceedance_Positions.txt and Exceedance_Summary.txt for the files
    under test: names [F], recs int32 [F, >= P, 8], elig [F, P], ge [F, P, 4, 2]; positions [(chrom, coordinate)], bases [P] (the panel's
    reference-base strings).  AF '%.6f', rates '%.4f', the median of the eligible normals '%.1f' (the mean of the two middle files)."""
    P, F = len(ref_code), len(names)
    prm = dict(min_alt_reads=min_alt_reads, min_vaf_pm=min_vaf_pm, min_normals=min_normals, max_normals=max_normals)
    elig, ge = np.asarray(elig).reshape(F, P), np.asarray(ge).reshape(F, P, 4, 2)
    cand = candidates(recs, elig, ge, **prm) if F else np.zeros((0, P, 4), bool)
    ev = ge[..., 0] != NA
    _, x, D = counts(np.asarray(recs)[:, :P])

    def per_1000(c, e):
        return "%.4f" % (1000.0 * float(c) / float(e) if e else 0.0)

    out = {}
    text = "sample\tchrom\tposition\tsubstitution\tXfw\tXrs\tFW\tBW\tAF\tElig\tGE_fw\tGE_rs\n"
    for f, p, y in zip(*np.nonzero(cand)):
        xf, xb, df, db = int(x[f, p, 0, y]), int(x[f, p, 1, y]), int(D[f, p, 0]), int(D[f, p, 1])
        af = "%.6f" % (float(xf + xb) / float(df + db)) if df + db else "NA"
        text += (f"{names[f]}\t{positions[p][0]}\t{positions[p][1]}\t{NT[ref_code[p]]}->{NT[y]}\t{xf}\t{xb}\t{df}\t{db}\t{af}\t{elig[f, p]}\t{ge[f, p, y, 0]}\t"
                 f"{ge[f, p, y, 1]}\n")
    out["Exceedance_Candidates.txt"] = text
    text = "sample\tEvaluated\tCandidates\tCandidates_per_1000\n"
    for f in range(F):
        text += f"{names[f]}\t{ev[f].sum()}\t{cand[f].sum()}\t{per_1000(cand[f].sum(), ev[f].sum())}\n"
    out["Exceedance_Samples.txt"] = text
    text = "chrom\tposition\treference\tMedianElig\tCand_A\tCand_C\tCand_G\tCand_T\n"
    col = np.sort(elig.astype(np.int64), axis=0)
    for p in range(P):
        median = "%.1f" % ((float(col[(F - 1) // 2, p]) + float(col[F // 2, p])) / 2.0) if F else "NA"
        text += f"{positions[p][0]}\t{positions[p][1]}\t{bases[p]}\t{median}\t" + "\t".join(str(int(cand[:, p, y].sum())) for y in range(4)) + "\n"
    out["Exceedance_Positions.txt"] = text
    out["Exceedance_Summary.txt"] = (
        f"normals={n_normals}\ntumours={n_tumours}\npositions={P}\npositions_with_reference={(np.asarray(ref_code) <= 3).sum()}\n"
        f"coverage_cutoff={coverage_cutoff}\ncalling_cutoff={calling_cutoff}\nmin_alt_reads={min_alt_reads}\nmin_vaf_pm={min_vaf_pm}\nmin_normals={min_normals}\n"
        f"max_normals={max_normals}\nskip_same_index={int(skip_same_index)}\nevaluated={ev.sum()}\ncandidates={cand.sum()}\n"
        f"candidates_per_1000={per_1000(cand.sum(), ev.sum())}\n")
    return out


def candidates(recs_t, elig, ge, **prm):
    """the candidate cells of whole rows: recs_t int32 [n_t, >= P, 8], elig [n_t, P], ge [n_t, P, 4, 2] -> bool [n_t, P, 4]"""
    P = np.asarray(elig).shape[1]
    _, x, D = counts(np.asarray(recs_t)[:, :P])
    x = x.transpose(0, 1, 3, 2)                                     # [n_t, P, 4, 2]
    depth = np.broadcast_to(D[:, :, None, :], x.shape)
    return candidate_cells(x, depth, np.asarray(elig)[:, :, None], ge, **prm)
