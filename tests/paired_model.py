"""The definition of the paired comparison -- TEST INFRASTRUCTURE, and the text that include/amplisolve_hip.h,
include/amplisolve_host.h, csrc/ampli_math.h and csrc/ampli_paired.hip restate.

Two count files of one patient, a and b, at one (position, strand, base):  k_a alternative reads among d_a (the sum of a's four counts
on the strand), k_b among d_b.  N = d_a + d_b, K = k_a + k_b, n = d_a, and X is hypergeometric: the number of alternative reads among
a's n when K alternative reads are dealt among N.  Only the primary record of (row, position) enters.

A cell is EVALUATED iff both records are present, all four strand depths (a and b, forward and backward) are >= depth_cutoff, the
reference code of the position is 0..3 and the base is not the reference base; every other cell holds NA (-999) on both strands.

Per strand the evaluated cell gets a signed score S, decided in integers by c = k_a N - K n:
  K == 0 or c == 0:  S = +0
  c > 0 (a's fraction is the higher):  p = P[X >= k_a],  S = +float32(-10 log10(max(p, 1e-10)))
  c < 0:                               p = P[X <= k_a],  S = -float32(-10 log10(max(p, 1e-10)))
  p >= 1 gives +0; -0 is never stored.

Here p is exact: a rational from math.comb where N <= EXACT_MAX_N, otherwise the first term from mpmath's loggamma at 50 digits and
the later terms from the exact integer ratios in 220-bit fixed point, summed until a term is below 2^-130 of the sum.

python -m tests.paired_model writes the recorded grid tests/golden/paired/hyper_grid.npz."""
import functools
import math
from fractions import Fraction

import numpy as np
from mpmath import mp

DPS = 50
EXACT_MAX_N = 300
NA = np.float32(-999.0)
ABSENT = np.iinfo(np.int32).min
D_MAX = 2 ** 31 - 1
_FIX = 220


def support(N, K, n):
    return max(0, n - (N - K)), min(K, n)


@functools.lru_cache(maxsize=1 << 16)
def _lfact(v):
    """ln v! at DPS + 15 digits (the depths and counts of a cohort come back again and again)"""
    with mp.workdps(DPS + 15):
        return mp.loggamma(v + 1)


def hyper_tail(N, K, n, k, up):
    """P[X >= k] (up) or P[X <= k]: a Fraction for N <= EXACT_MAX_N, else an mpf good to ~35 digits.  k inside the support."""
    lo, hi = support(N, K, n)
    assert 0 <= n <= N and 0 <= K <= N and lo <= k <= hi
    if N <= EXACT_MAX_N:
        xs = range(k, hi + 1) if up else range(lo, k + 1)
        return Fraction(sum(math.comb(K, x) * math.comb(N - K, n - x) for x in xs), math.comb(N, n))
    with mp.workdps(DPS + 15):
        lg = _lfact
        lp = (lg(K) - lg(k) - lg(K - k) + lg(N - K) - lg(n - k) - lg(N - K - n + k)) - (lg(N) - lg(n) - lg(N - n))
        first = mp.exp(lp)
    if up:
        A, B, C, D = K - k, n - k, k + 1, N - K - n + k + 1
    else:
        A, B, C, D = k, N - K - n + k, K - k + 1, n - k + 1
    t = s = 1 << _FIX
    while A > 0 and B > 0:
        t = t * (A * B) // (C * D)  # Python integers: a sum that first rises towards the mode has all the head room it needs
        s += t
        A, B, C, D = A - 1, B - 1, C + 1, D + 1
        if t < (s >> 130) and A * B < C * D:
            break
    with mp.workdps(DPS):
        return first * mp.mpf(s) / mp.mpf(1 << _FIX)


def as_mpf(p):
    with mp.workdps(DPS):
        return mp.mpf(p.numerator) / mp.mpf(p.denominator) if isinstance(p, Fraction) else mp.mpf(p)


@functools.lru_cache(maxsize=None)
def pair_s_exact(k_a, d_a, k_b, d_b):
    """the signed score before it is rounded to a float: an mpf (or the exact 0)"""
    k_a, d_a, k_b, d_b = int(k_a), int(d_a), int(k_b), int(d_b)
    assert 0 <= k_a <= d_a and 0 <= k_b <= d_b
    N, K, n = d_a + d_b, k_a + k_b, d_a
    c = k_a * N - K * n
    if K == 0 or c == 0:
        return mp.mpf(0)
    p = hyper_tail(N, K, n, k_a, c > 0)
    with mp.workdps(DPS):
        p = as_mpf(p)
        if p >= 1:
            return mp.mpf(0)
        q = -10 * mp.log10(max(p, mp.mpf(10) ** -10))
        return q if c > 0 else -q


def pair_s(k_a, d_a, k_b, d_b):
    v = np.float32(float(pair_s_exact(k_a, d_a, k_b, d_b)))
    return np.float32(0.0) if v == 0 else v


def hyper_variance(k_a, d_a, k_b, d_b):
    """n (K / N) (1 - K / N) (N - n) / (N - 1) as float64 arrays"""
    n, N, K = np.asarray(d_a, np.float64), np.asarray(d_a, np.float64) + np.asarray(d_b, np.float64), np.asarray(k_a, np.float64) + np.asarray(k_b, np.float64)
    return n * (K / N) * (1.0 - K / N) * (N - n) / np.maximum(N - 1.0, 1.0)


def score_model(recs_a, recs_b, P, pairs, ref_code, cutoff):
    """recs int32 [n][>= P][8] (primary slots), pairs [(row in a, row in b)] -> s float32 [n_pairs][P][4][2] and float64 of the same
    shape (the unrounded S); a row index outside its chunk makes the pair all NA"""
    recs_a, recs_b = np.asarray(recs_a, np.int64)[:, :P], np.asarray(recs_b, np.int64)[:, :P]
    s = np.full((len(pairs), P, 4, 2), NA, np.float32)
    s64 = np.full((len(pairs), P, 4, 2), float(NA), np.float64)
    for q, (ia, ib) in enumerate(pairs):
        if not (0 <= ia < recs_a.shape[0] and 0 <= ib < recs_b.shape[0]):
            continue
        for p in range(P):
            a, b = recs_a[ia, p], recs_b[ib, p]
            if a[0] == ABSENT or b[0] == ABSENT or ref_code[p] > 3:
                continue
            Da, Db = (int(a[0:4].sum()), int(a[4:8].sum())), (int(b[0:4].sum()), int(b[4:8].sum()))
            if min(Da) < cutoff or min(Db) < cutoff:
                continue
            for y in range(4):
                if y == ref_code[p]:
                    continue
                for st in range(2):
                    v = float(pair_s_exact(int(a[st * 4 + y]), Da[st], int(b[st * 4 + y]), Db[st]))
                    s64[q, p, y, st] = v
                    s[q, p, y, st] = pair_s(int(a[st * 4 + y]), Da[st], int(b[st * 4 + y]), Db[st])
    return s, s64


VERDICTS = ("HIGHER_IN_A", "LOWER_IN_A", "SHARED", "UNRESOLVED")


def verdict(s_fw, s_bw, vaf_a, vaf_b, q_min, min_vaf):
    if s_fw >= q_min and s_bw >= q_min:
        return "HIGHER_IN_A"
    if s_fw <= -q_min and s_bw <= -q_min:
        return "LOWER_IN_A"
    if vaf_a >= min_vaf and vaf_b >= min_vaf:
        return "SHARED"
    return "UNRESOLVED"


def cells(recs_a, recs_b, pairs, s, P, q_min, min_vaf):
    """every evaluated cell whose pooled VAF in a or in b is >= min_vaf: (pair, position, base, counts a, counts b, vaf a, vaf b, verdict),
    and per pair [evaluated, HIGHER_IN_A, LOWER_IN_A, SHARED, UNRESOLVED] over the listed cells"""
    rows, per_pair = [], []
    for q, (ia, ib) in enumerate(pairs):
        cnt = [0, 0, 0, 0, 0]
        for p in range(P):
            a, b = recs_a[ia, p].astype(np.int64), recs_b[ib, p].astype(np.int64)
            for y in range(4):
                if s[q, p, y, 0] == NA:
                    continue
                cnt[0] += 1
                da, db = int(a.sum()), int(b.sum())
                va = float(a[y] + a[4 + y]) / da if da else 0.0
                vb = float(b[y] + b[4 + y]) / db if db else 0.0
                if not (va >= min_vaf or vb >= min_vaf):
                    continue
                v = verdict(s[q, p, y, 0], s[q, p, y, 1], va, vb, q_min, min_vaf)
                cnt[1 + VERDICTS.index(v)] += 1
                rows.append((q, p, y, a, b, va, vb, v))
        per_pair.append(cnt)
    return rows, per_pair


def format_files(names_a, names_b, positions, ref_code, recs_a, recs_b, pairs, s, params):
    """the command line's three files as text.  names_a / names_b: the files of chunk a / b as the Summary names samples; positions
    [(chrom, coordinate)]; recs int32 [n][>= P][8]; pairs [(row in a, row in b)]; s float32 [n_pairs][P][4][2]; params: depth_cutoff,
    q_min, min_vaf"""
    P, q_min, min_vaf = len(positions), float(params["q_min"]), float(params["min_vaf"])
    rows, per_pair = cells(recs_a, recs_b, pairs, s, P, q_min, min_vaf)
    out = "a\tb\tchrom\tposition\tsubstitution\tXfw_a\tXrs_a\tFW_a\tBW_a\tXfw_b\tXrs_b\tFW_b\tBW_b\tVAF_a\tVAF_b\tS_fw\tS_rs\tVerdict\n"
    for q, p, y, a, b, va, vb, v in rows:
        ia, ib = pairs[q]
        out += (f"{names_a[ia]}\t{names_b[ib]}\t{positions[p][0]}\t{positions[p][1]}\t{'ACGT'[ref_code[p]]}->{'ACGT'[y]}\t{a[y]}\t{a[4 + y]}\t{a[:4].sum()}\t"
                f"{a[4:].sum()}\t{b[y]}\t{b[4 + y]}\t{b[:4].sum()}\t{b[4:].sum()}\t{va:.6f}\t{vb:.6f}\t{s[q, p, y, 0]:.4f}\t{s[q, p, y, 1]:.4f}\t{v}\n")
    pp = "a\tb\tEvaluated\tHigherInA\tLowerInA\tShared\tUnresolved\n"
    tot = [0, 0, 0, 0, 0]
    for (ia, ib), c in zip(pairs, per_pair):
        pp += f"{names_a[ia]}\t{names_b[ib]}\t" + "\t".join(str(v) for v in c) + "\n"
        tot = [x + y for x, y in zip(tot, c)]
    summary = (f"pairs={len(pairs)}\npositions={P}\ndepth_cutoff={params['depth_cutoff']}\nq_min={q_min:g}\nmin_vaf={min_vaf:g}\nevaluated={tot[0]}\n"
               f"higher_in_a={tot[1]}\nlower_in_a={tot[2]}\nshared={tot[3]}\nunresolved={tot[4]}\n")
    return {"Paired_Cells.txt": out, "Paired_Pairs.txt": pp, "Paired_Summary.txt": summary}


# ---- the recorded grid (tests/golden/paired/hyper_grid.npz): python -m tests.paired_model writes it -----------------------------------

GRID_D = (1, 2, 7, 100, 5000, 65535, 1000003, D_MAX)


def _clamp_cases(d_a, d_b, k_b):
    """k_a around the count where P[X >= k_a] crosses 1e-10, and the mirrored tables (the clamp from both sides, on both signs)"""
    k = k_b * d_a // d_b + 1
    lim = mp.mpf(10) ** -10
    while k < d_a and as_mpf(hyper_tail(d_a + d_b, k + k_b, d_a, k, True)) >= lim:
        k += 1
    out = [(kk, d_a, k_b, d_b) for kk in (k - 2, k - 1, k, k + 1) if 0 <= kk <= d_a]
    return out + [(kb, db, ka, da) for ka, da, kb, db in out]


def grid_cases(seed=20, n_random=20000):
    """(k_a, d_a, k_b, d_b) of the grid, c == 0 and K == 0, the clamp and n_random random tables, as int32 arrays"""
    rng = np.random.default_rng(seed)
    out = []
    for d_a in GRID_D:
        for d_b in sorted({d_a, max(1, d_a // 1000), min(D_MAX, d_a * 1000)}):
            N, n = d_a + d_b, d_a
            for K in sorted({0, 1, 2, 3, N // 1000, N // 10, N // 2, N - N // 10, N - 1, N}):
                lo, hi = support(N, K, n)
                m = n * K // N
                ks = {0, 1, 2, m - 2, m - 1, m, m + 1, m + 2, m + 3, lo, lo + 1, hi - 1, hi}
                out += [(k, d_a, K - k, d_b) for k in sorted(ks) if lo <= k <= hi]
    out += [(5, 100, 50, 1000), (0, 100, 0, 7), (0, 1, 0, 1), (3, 9, 3, 9), (1 << 20, D_MAX, 1 << 20, D_MAX), (D_MAX, D_MAX, D_MAX, D_MAX), (0, D_MAX, 0, 3)]
    out += [((1 << 20) + 5000, D_MAX, 1 << 20, D_MAX), (1 << 20, D_MAX, (1 << 20) + 5000, D_MAX)]  # the longest sum of the prototype
    for d_a, d_b, k_b in ((6000, 5000, 0), (6000, 5000, 5), (100, 100, 0), (40, 3000, 3), (200000, 2000, 9), (1000003, 1000003, 700), (D_MAX, D_MAX, 40)):
        out += _clamp_cases(d_a, d_b, k_b)
    d = np.exp(rng.uniform(0, math.log(D_MAX), (n_random, 2))).astype(np.int64)
    f = np.exp(rng.uniform(math.log(1e-4), math.log(0.9), n_random))
    z = rng.normal(0, 2, (n_random, 2))
    k = np.clip(np.rint(d * f[:, None] + z * np.sqrt(d * (f * (1 - f))[:, None] + 0.3)), 0, d).astype(np.int64)
    out += [(int(k[i, 0]), int(d[i, 0]), int(k[i, 1]), int(d[i, 1])) for i in range(n_random)]
    return tuple(np.array([c[j] for c in out], np.int32) for j in range(4))


def write_golden(path):
    k_a, d_a, k_b, d_b = grid_cases()
    s = np.array([float(pair_s_exact(k_a[i], d_a[i], k_b[i], d_b[i])) for i in range(len(k_a))], np.float64)
    np.savez_compressed(path, k_a=k_a, d_a=d_a, k_b=k_b, d_b=d_b, s=s)
    return len(s)


if __name__ == "__main__":
    import os

    dst = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "paired")
    os.makedirs(dst, exist_ok=True)
    print(write_golden(os.path.join(dst, "hyper_grid.npz")), "cases")
