"""The definition of the cross-sample contamination check in plain numpy -- TEST INFRASTRUCTURE, the yardstick of
contamination_kernel, ampli_contamination_estimate and AmpliSolveContamination.

The nine sums of an ordered pair come from matrix products of indicator matrices (one per presence set of the recipient, one per
presence set and zygosity of the source) with count matrices, not from bit planes: the model and the kernel share nothing.  The plane
bits of a record are those of tests/concordance_model.classify.  The products run in float64 over integers; every result is asserted to
be below 2^53, where sums of non-negative integers are exact in any order.  The estimate is Python float arithmetic, one rounded
operation per line of the contract."""
import math

import numpy as np

from tests.concordance_model import ABSENT, DEFAULTS, H, V

SITES_HOM, ALT_HOM, DEPTH_HOM, SITES_HET, ALT_HET, DEPTH_HET, SITES_BG, ALT_BG, DEPTH_BG = range(9)  # AMPLI_CONTAM_*
UNDETERMINED, CLEAN, CONTAMINATED = 0, 1, 2  # AMPLI_CONTAM_STATUS_*
STATUS = ("UNDETERMINED", "CLEAN", "CONTAMINATED")
EXACT = float(1 << 53)


def counts(recs_a):
    """int32 [n, >= P, 8] -> n[Y] int64 [n, P', 4] and d int64 [n, P']; an absent record counts as zeros"""
    r = np.asarray(recs_a).astype(np.int64)
    n = np.where((r[..., 0] != ABSENT)[..., None], r[..., :4] + r[..., 4:], 0)
    return n, n.sum(-1)


def sums(recs_a, bits_a, bits_b):
    """recs_a int32 [n, P, 8] (the recipients' primary records), bits_a uint8 [n, P], bits_b uint8 [n_b, P] -> int64 [n, n_b, 9]"""
    bits_a, bits_b = np.asarray(bits_a), np.asarray(bits_b)
    n, P = bits_a.shape
    n_b = bits_b.shape[0]
    assert bits_b.shape[1] == P and np.asarray(recs_a).shape[:2] == (n, P)
    cnt, d = counts(recs_a)
    f = lambda m: np.ascontiguousarray(m, dtype=np.float64)
    hom_a = ((bits_a & V) != 0) & ((bits_a & H) == 0)
    set_a, set_b = (bits_a >> 1) & 15, (bits_b >> 1) & 15
    vb, hb = (bits_b & V) != 0, (bits_b & H) != 0
    out = np.zeros((n, n_b, 9), np.float64)
    for sa in range(16):
        ia = hom_a & (set_a == sa)
        if not ia.any():
            continue
        lacks = [y for y in range(4) if not (sa >> y) & 1]      # the bases with ~A_Y
        one, depth = f(ia), f(ia * d)
        other = f(ia * cnt[..., lacks].sum(-1))                 # sum of n[Y] over the Y with ~A_Y
        for sb in range(16):
            on = [y for y in lacks if (sb >> y) & 1]            # o[Y]: b carries Y, a does not
            for het in (False, True):
                jb = vb & (hb == het) & (set_b == sb)
                if not jb.any():
                    continue
                jt = f(jb).T
                if on:
                    alt = f(ia * cnt[..., on].sum(-1))
                    k = (SITES_HET, ALT_HET, DEPTH_HET) if het else (SITES_HOM, ALT_HOM, DEPTH_HOM)
                    out[..., k[0]] += one @ jt
                    out[..., k[1]] += alt @ jt
                    out[..., k[2]] += (len(on) if het else 1) * (depth @ jt)
                else:
                    out[..., SITES_BG] += one @ jt
                    out[..., ALT_BG] += other @ jt
                    out[..., DEPTH_BG] += depth @ jt
    assert (out == np.rint(out)).all() and (out >= 0).all() and (out < EXACT).all()
    return out.astype(np.int64)


def estimate(s):
    """the nine sums of one pair -> (fraction, se, e) in double, one rounding per operation, in the contract's order"""
    s = [int(x) for x in s]
    alt = float(s[ALT_HOM] + s[ALT_HET])
    slots = float(s[DEPTH_HOM] + s[DEPTH_HET])
    den = float(s[DEPTH_HOM]) + 0.5 * float(s[DEPTH_HET])
    e = float(s[ALT_BG]) / (3.0 * float(s[DEPTH_BG])) if s[DEPTH_BG] > 0 else 0.0
    prod = e * slots
    num = alt - prod
    if not den > 0:
        return math.nan, math.nan, e
    q = num / den
    return (q if q > 0.0 else 0.0), math.sqrt(alt) / den, e


def status(s, min_sites, min_fraction):
    if int(s[SITES_HOM]) + int(s[SITES_HET]) < min_sites:
        return UNDETERMINED
    return CONTAMINATED if estimate(s)[0] >= min_fraction else CLEAN


def statuses(S, min_sites, min_fraction):
    return np.array([[status(S[i, j], min_sites, min_fraction) for j in range(S.shape[1])] for i in range(S.shape[0])])


def _f5(x):
    return "NA" if x != x else "%.5f" % x


def format_files(names, n_normals, S, min_sites, min_fraction, prm=None):
    """the three files of AmpliSolveContamination from the N x N x 9 sums of normals-then-tumours: (samples, pairs, summary)"""
    prm = dict(DEFAULTS, **(prm or {}))
    N = len(names)
    st = statuses(S, min_sites, min_fraction)
    est = [[estimate(S[i, j]) for j in range(N)] for i in range(N)]
    samples = "Sample\tSet\tHomSites\tBackground\tSource\tSites\tFraction\tSE\tStatus\n"
    for i in range(N):
        best = -1
        rank = lambda j: est[i][j][0] if est[i][j][0] == est[i][j][0] else -1.0  # a pair without depth ranks last
        for j in range(N):
            if st[i, j] == UNDETERMINED:
                continue
            if best < 0 or rank(j) > rank(best):  # the first source in order wins a tie
                best = j
        samples += f"{names[i]}\t{'N' if i < n_normals else 'T'}\t{int(S[i, i, SITES_BG])}\t{'%.6f' % est[i][i][2]}\t"
        if best < 0:
            samples += "NA\tNA\tNA\tNA\tUNDETERMINED\n"
        else:
            samples += (f"{names[best]}\t{int(S[i, best, SITES_HOM]) + int(S[i, best, SITES_HET])}\t{_f5(est[i][best][0])}\t{_f5(est[i][best][1])}\t"
                        f"{STATUS[st[i, best]]}\n")
    pairs = "Recipient\tSource\tSitesHom\tAltHom\tDepthHom\tSitesHet\tAltHet\tDepthHet\tSitesBg\tAltBg\tDepthBg\tFraction\tSE\n"
    by = [0, 0, 0]
    for i in range(N):
        for j in range(N):
            if i == j:
                continue
            by[st[i, j]] += 1
            if st[i, j] == CONTAMINATED:
                pairs += f"{names[i]}\t{names[j]}\t" + "\t".join(str(int(x)) for x in S[i, j]) + f"\t{_f5(est[i][j][0])}\t{_f5(est[i][j][1])}\n"
    summary = (f"normals={n_normals}\ntumours={N - n_normals}\n" + "".join(f"{k}={prm[k]}\n" for k in DEFAULTS) +
               f"min_sites={min_sites}\nmin_fraction={'%g' % min_fraction}\npairs_contaminated={by[CONTAMINATED]}\npairs_clean={by[CLEAN]}\n"
               f"pairs_undetermined={by[UNDETERMINED]}\n")
    return samples, pairs, summary
