"""The dispersion of a panel of normals, the definition -- TEST INFRASTRUCTURE.

A cell is (strand, base, position).  Its qualifying records are the ones cnt[nt][p] of the error table counts (EE:1592-1606): every
present record of every normal at p, primary and extra occurrences alike, with FW >= and BW >= coverage_cutoff and both fp32 strand
fractions of the base <= 0.05.  An RD column of the line's own plays no part in that gate.  With k_i the record's count of the base on
the strand, d_i the strand's depth, K = sum k_i, D = sum d_i, r = K / D over the n qualifying records:

    X2  = sum (k_i - r d_i)^2 / (r d_i) = (D / K) sum k_i^2 / d_i - K
    phi = X2 / (n - 1)
    z   = (X2 - (n - 1)) / sqrt(V),   V = 2 (n - 1) + (D sum 1/d_i - n^2 - 2 n + 2) / K

A cell with n < 2 or K < 2 is FEW (status 1): X2 = sum 1/d = z = phi = 0 and it contributes to no per-sample sum.  Given K the k_i are
multinomial with probabilities d_i / D under the pooled rate; the mean n - 1 and the variance V are Haldane's exact moments of X2.

Everything up to X2, sum 1/d and V is exact rational arithmetic (fractions.Fraction over Python integers); floats appear where a number
leaves: float(X2), float(sum 1/d), z = float(X2 - (n - 1)) / sqrt(float(V)).  The per-sample sums run over up to 8 (P + E) terms with
unrelated denominators: each term is formed exactly as a ratio of integers, rounded once to a double, and the doubles are added with
math.fsum (an exactly rounded sum): 2^-53 relative per non-negative term, far below the 1e-10 the sums are held to.
"""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

ABSENT = np.iinfo(np.int32).min
OK, FEW, HIGH = 0, 1, 0x40


def qualifying(recs, cov):
    """bool [S][R][4]: the record's counts of base nt go into the threshold sums (EE:1592-1606)"""
    recs = np.asarray(recs, np.int64)
    present = recs[:, :, 0] != ABSENT
    r = np.where(present[:, :, None], recs, 0)
    fw, bw = r[:, :, 0:4].sum(axis=2), r[:, :, 4:8].sum(axis=2)
    with np.errstate(divide="ignore", invalid="ignore"):
        af_fw = (r[:, :, 0:4].astype(np.float32) / fw.astype(np.float32)[:, :, None]).astype(np.float64)
        af_bw = (r[:, :, 4:8].astype(np.float32) / bw.astype(np.float32)[:, :, None]).astype(np.float64)
    cov_ok = present & (fw >= cov) & (bw >= cov)
    return cov_ok[:, :, None] & (af_fw <= 0.05) & (af_bw <= 0.05)


def haldane_variance(n, K, D, rinv):
    """exact: n, K, D integers, rinv = sum 1/d a Fraction"""
    return 2 * (n - 1) + (D * rinv - n * n - 2 * n + 2) / Fraction(K)


def cell_exact(k, d):
    """one cell from its qualifying records' counts k and depths d (sequences of Python ints): n, K, D and, exact, X2, sum 1/d, V
    (None, None, None when FEW)"""
    n, K, D = len(k), sum(k), sum(d)
    if n < 2 or K < 2:
        return n, K, D, None, None, None
    by_d = {}
    inv = {}
    for ki, di in zip(k, d):
        by_d[di] = by_d.get(di, 0) + ki * ki
        inv[di] = inv.get(di, 0) + 1
    x2 = Fraction(D, K) * sum(Fraction(v, di) for di, v in by_d.items()) - K
    rinv = sum(Fraction(m, di) for di, m in inv.items())
    return n, K, D, x2, rinv, haldane_variance(n, K, D, rinv)


def dispersion_model(recs, P, cov, E=0, ext_pos=None, z_cutoff=4.0):
    """recs int32 [S][P+E][8] (the dense interchange layout), ext_pos [E] the position of every extra occurrence.  Returns n [4][P],
    K, D int64 [2][4][P]; x2, rinv, z float64, phi float32, status uint8, each [2][4][P]; counts [4] (cells OK, FEW, HIGH, positions
    with a HIGH cell); sample_x2, sample_expect float64 [S], sample_terms int64 [S]; sample_scale [S] = sum (k + r d) over the same
    terms (what sample_x2's tolerance is scaled with)."""
    recs = np.ascontiguousarray(recs, np.int64)
    S, R = recs.shape[0], recs.shape[1]
    assert R == P + E
    pos = np.arange(R)
    if E:
        pos[P:] = np.asarray(ext_pos, np.int64)
    q = qualifying(recs, cov)
    fw = np.where(recs[:, :, 0] != ABSENT, recs[:, :, 0:4].sum(axis=2), 0)
    bw = np.where(recs[:, :, 0] != ABSENT, recs[:, :, 4:8].sum(axis=2), 0)
    n = np.zeros((4, P), np.int64)
    K = np.zeros((2, 4, P), np.int64)
    D = np.zeros((2, 4, P), np.int64)
    x2 = np.zeros((2, 4, P), np.float64)
    rinv = np.zeros((2, 4, P), np.float64)
    z = np.zeros((2, 4, P), np.float64)
    phi = np.zeros((2, 4, P), np.float32)
    status = np.full((2, 4, P), FEW, np.uint8)
    terms_x2 = [[] for _ in range(S)]
    terms_ex = [[] for _ in range(S)]
    terms_sc = [[] for _ in range(S)]
    # records of every position, by position: (sample, record) pairs in any order -- the definition is a sum
    order = np.argsort(pos, kind="stable")
    bounds = np.searchsorted(pos[order], np.arange(P + 1))
    for p in range(P):
        rr = order[bounds[p]:bounds[p + 1]]
        for nt in range(4):
            ss, ri = np.nonzero(q[:, rr, nt])
            if len(ss) == 0:
                continue
            ri = rr[ri]
            n[nt, p] = len(ss)
            for st, depth in ((0, fw), (1, bw)):
                k = [int(v) for v in recs[ss, ri, st * 4 + nt]]
                d = [int(v) for v in depth[ss, ri]]
                nn, KK, DD, X2, RI, V = cell_exact(k, d)
                K[st, nt, p], D[st, nt, p] = KK, DD
                if X2 is None:
                    continue
                x2[st, nt, p] = float(X2)
                rinv[st, nt, p] = float(RI)
                zz = float(X2 - (nn - 1)) / math.sqrt(float(V))
                z[st, nt, p] = zz
                phi[st, nt, p] = np.float32(float(X2 / (nn - 1)))
                status[st, nt, p] = HIGH if zz >= z_cutoff else OK
                for s, ki, di in zip(ss, k, d):
                    terms_x2[s].append((ki * DD - KK * di) ** 2 / (KK * DD * di))  # int / int: correctly rounded
                    terms_ex[s].append((DD - di) / DD)
                    terms_sc[s].append((ki * DD + KK * di) / DD)
    ok = status != FEW
    high = (status & HIGH) != 0
    counts = np.array([ok.sum(), (~ok).sum(), high.sum(), high.any(axis=(0, 1)).sum()], np.int64)
    return dict(n=n, K=K, D=D, x2=x2, rinv=rinv, z=z, phi=phi, status=status, counts=counts,
                sample_x2=np.array([math.fsum(t) for t in terms_x2]), sample_expect=np.array([math.fsum(t) for t in terms_ex]),
                sample_scale=np.array([math.fsum(t) for t in terms_sc]), sample_terms=np.array([len(t) for t in terms_x2], np.int64))
