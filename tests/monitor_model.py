"""The definition of tumour-informed monitoring -- TEST INFRASTRUCTURE, and the text that include/amplisolve_hip.h,
csrc/ampli_math.h and DESIGN 24 restate.  Pooled evidence over the cells of a variant list: is a patient's tumour, known as a list of
somatic variants, in this plasma sample at all?

  Lists.  A CSR: list_off uint32 [L + 1] and list_cell uint32 [W], an entry c = 4 p + y (position index p, base y).  Lists may be empty,
    may overlap and may name a cell several times; a cell named twice counts twice.  An entry with p >= P is none.  Offsets are cut to
    [0, W].
  Evaluated entry of sample row s, from the PRIMARY record only (slot p < P).  All of these hold: the record is present; D_fw >=
    coverage_cutoff and D_bw >= coverage_cutoff, each the sum of the strand's four counts; ref_code[p] in 0..3 and y != it; e_fw =
    thr[0][y][p] and e_bw = thr[1][y][p] are both finite and >= 0 (so not -1, "no estimate"); 1000 (k_fw + k_bw) <= max_vaf_pm (D_fw +
    D_bw) in integers, k the strand's count of base y.  e == 0 is replaced by float32(0.0010008).
  Sums per (sample, list).  Six integers -- N_EVAL, N_SEEN (evaluated entries with k_fw + k_bw >= 1), K_FW, K_BW, D_FW, D_BW -- and two
    doubles Lambda_fw, Lambda_bw, each the sum of double(d_st) * double(e_st).  The order of the double additions is part of the
    definition: lane j of 64 takes the list's entries j, j + 64, ... in ascending order and adds each product to an accumulator that
    starts at +0.0 (an entry that is not evaluated adds nothing); the 64 accumulators are combined by the butterfly x += x[lane ^ off]
    for off = 32, 16, 8, 4, 2, 1.
  Pooled score per strand.  Q = 0 for p >= 1, else -10 log10(max(p, 1e-10)), p = P[X >= K] for X Poisson of mean Lambda: K == 0 gives
    0, Lambda == 0 with K > 0 gives 100; N_EVAL == 0 gives NA (-1) on both strands.  Here the tail is summed in mpmath at 50 digits.
  Matched random controls, replicate r (global index) of list l.  Entry i (0-based within the list) at (p, y) with g = ref_code[p]
    becomes (p', y); p' is drawn from the m candidates of g (cand_off uint32 [5], cand_pos: positions grouped by reference base):
    word = output word 0 of Philox4x32-10 with counter (i, r, l, TAG) and key (low word, high word of the 64-bit seed), p' =
    cand[(word * m) >> 32].  No control entry where p >= P, g > 3, m == 0 or p' >= P.  The multiply-high draw favours some candidates by
    less than m / 2^32.  A control list depends on (seed, l, r) only; its sums are formed exactly as above.
  Verdicts.  NOT_EVALUABLE if N_EVAL < min_variants; else DETECTED iff N_SEEN >= min_seen and Q_fw >= q_min and Q_bw >= q_min; else
    NOT_DETECTED.  Excess fraction of a strand: max(0, (K - Lambda) / D), 0 for D <= 0.  Empirical p of an own pair: (1 + n_ge) /
    (R + 1), n_ge the controls whose min(Q_fw, Q_bw) >= the observed min.  Pooled limit of detection: per strand the smallest K >=
    floor(Lambda) + 1 whose pooled Q reaches q_min, found by walking upwards for at most LOD_MAX_EVALS evaluations; the larger of the
    strands' (K_min - Lambda) / D, -1 where a strand has none or no depth."""
from __future__ import annotations

import functools
import math

import mpmath as mp
import numpy as np

from tests.dilution_model import philox

ABSENT = np.iinfo(np.int32).min
N_EVAL, N_SEEN, K_FW, K_BW, D_FW, D_BW, SUMS = 0, 1, 2, 3, 4, 5, 6
NA = np.float32(-1.0)
NOT_EVALUABLE, NOT_DETECTED, DETECTED = 0, 1, 2
TAG = 0x4D4F4E31
LOD_MAX_EVALS = 4096
E0 = np.float32(0.0010008)
DPS = 50
LANES = np.arange(64)


def butterfly(acc):
    """the 64 accumulators combined: x += x[lane ^ off] for off = 32, 16, 8, 4, 2, 1; every lane ends with the same double"""
    acc = np.array(acc, np.float64)
    assert acc.shape == (64,)
    for off in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[LANES ^ off]
    return acc[0]


def thr_ok(e):
    e = np.float32(e)
    return bool(np.isfinite(e) and e >= 0)


def cut(list_off, l, W):
    off = min(int(list_off[l]), W)
    end = min(int(list_off[l + 1]), W)
    return off, max(end, off)


def entries(list_off, list_cell, l):
    """the entries of list l as (p, y) pairs"""
    off, end = cut(list_off, l, len(list_cell))
    return [(int(c) >> 2, int(c) & 3) for c in np.asarray(list_cell[off:end], np.int64)]


def entry_sums(row, P, thr, ref_code, ent, cov, max_vaf_pm):
    """one (row, list): row int [>= P][8], ent a list of (p, y) or None -> (six Python integers, Lambda_fw, Lambda_bw)"""
    thr = np.asarray(thr, np.float32).reshape(2, 4, P)
    s = [0] * SUMS
    lf, lb = np.zeros(64, np.float64), np.zeros(64, np.float64)
    for i, e in enumerate(ent):
        if e is None:
            continue
        p, y = e
        if p >= P or ref_code[p] > 3 or y == ref_code[p]:
            continue
        ef, eb = thr[0, y, p], thr[1, y, p]
        if not (thr_ok(ef) and thr_ok(eb)):
            continue
        r = [int(x) for x in row[p]]
        if r[0] == ABSENT:
            continue
        FW, BW, kf, kb = sum(r[:4]), sum(r[4:]), r[y], r[4 + y]
        if FW < cov or BW < cov or 1000 * (kf + kb) > max_vaf_pm * (FW + BW):
            continue
        s[N_EVAL] += 1
        s[N_SEEN] += kf + kb >= 1
        s[K_FW] += kf
        s[K_BW] += kb
        s[D_FW] += FW
        s[D_BW] += BW
        lf[i & 63] = lf[i & 63] + np.float64(FW) * np.float64(E0 if ef == 0 else ef)
        lb[i & 63] = lb[i & 63] + np.float64(BW) * np.float64(E0 if eb == 0 else eb)
    return s, butterfly(lf), butterfly(lb)


def sums_model(recs, P, thr, ref_code, list_off, list_cell, cov=100, max_vaf_pm=1000):
    """recs int32 [n][>= P][8] -> sums int64 [n][L][6], lam float64 [n][L][2]"""
    n, L = len(recs), len(list_off) - 1
    sums, lam = np.zeros((n, L, SUMS), np.int64), np.zeros((n, L, 2), np.float64)
    for l in range(L):
        ent = entries(list_off, list_cell, l)
        for s in range(n):
            sums[s, l], lam[s, l, 0], lam[s, l, 1] = entry_sums(recs[s], P, thr, ref_code, ent, cov, max_vaf_pm)
    return sums, lam


def control_draw(i, r, l, seed, m):
    """(word * m) >> 32 for arrays (or scalars) of entry indices i"""
    w = philox(i, r, l, TAG, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)[0]
    return (np.asarray(w, np.uint64) * np.uint64(m)) >> np.uint64(32)


def control_entries(P, ref_code, ent, cand_off, cand_pos, l, r, seed):
    """the control list of replicate r of list l: (p', y) or None per entry; it does not depend on the sample"""
    out = []
    n_cand = len(cand_pos)
    words = philox(np.arange(len(ent), dtype=np.uint64), r, l, TAG, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)[0] if ent else []
    for i, (p, y) in enumerate(ent):
        e = None
        if p < P and ref_code[p] <= 3:
            g = int(ref_code[p])
            lo = min(int(cand_off[g]), n_cand)
            hi = max(min(int(cand_off[g + 1]), n_cand), lo)
            if hi > lo:
                pp = int(cand_pos[lo + ((int(words[i]) * (hi - lo)) >> 32)])
                if pp < P:
                    e = (pp, y)
        out.append(e)
    return out


def controls_model(recs, P, thr, ref_code, list_off, list_cell, pairs, cand_off, cand_pos, R, first_rep, seed, cov=100, max_vaf_pm=1000):
    """-> sums int64 [n_pairs][R][6], lam float64 [n_pairs][R][2]; a pair with a row or list out of range is all zero"""
    n, L = len(recs), len(list_off) - 1
    sums, lam = np.zeros((len(pairs), R, SUMS), np.int64), np.zeros((len(pairs), R, 2), np.float64)
    for q, (row, l) in enumerate(pairs):
        if not (0 <= row < n and 0 <= l < L):
            continue
        ent = entries(list_off, list_cell, l)
        for k in range(R):
            ctl = control_entries(P, ref_code, ent, cand_off, cand_pos, int(l), first_rep + k, seed)
            sums[q, k], lam[q, k, 0], lam[q, k, 1] = entry_sums(recs[row], P, thr, ref_code, ctl, cov, max_vaf_pm)
    return sums, lam


def candidates(ref_code):
    """cand_off uint32 [5], cand_pos uint32: every position of the panel, grouped by reference base (a code above 3 is in no class)"""
    ref_code = np.asarray(ref_code)
    parts = [np.nonzero(ref_code == g)[0] for g in range(4)]
    return np.concatenate([[0], np.cumsum([len(x) for x in parts])]).astype(np.uint32), np.concatenate(parts).astype(np.uint32)


# ---- the pooled score ------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def pois_tail(K, lam):
    """P[X >= K] for X Poisson of mean lam (a double, taken exactly) as an mpf: K <= 0 gives 1, lam <= 0 gives 0; above the mean the sum
    from K upwards until what is left is below 1e-30 of it, else 1 - the sum from K - 1 downwards until a term is below 1e-45"""
    K = int(K)
    with mp.workdps(DPS):
        if K <= 0:
            return mp.mpf(1)
        if not lam > 0:
            return mp.mpf(0)
        m = mp.mpf(lam)

        def pmf(j):
            return mp.exp(j * mp.log(m) - m - mp.loggamma(j + 1))

        if K > lam:
            t = pmf(K)
            sm, j, eps = t, K, mp.mpf(10) ** -30
            while True:
                r = m / (j + 1)
                if t * r < eps * sm * (1 - r):
                    return sm
                t *= r
                sm += t
                j += 1
        j = K - 1
        t = pmf(j)
        sm, tiny = t, mp.mpf(10) ** -45
        while j > 0 and t > tiny:
            t *= j / m
            sm += t
            j -= 1
        return 1 - sm if sm < 1 else mp.mpf(0)


def q_exact(n_eval, K, lam):
    """the pooled Q of one strand before it is rounded to a float, as a Python float (the rounding of a 50-digit value)"""
    if n_eval <= 0:
        return -1.0
    p = pois_tail(int(K), float(lam))
    with mp.workdps(DPS):
        if p >= 1:
            return 0.0
        return float(-10 * mp.log10(max(p, mp.mpf(10) ** -10)))


def score_model(sums, lam):
    """sums [..., 6], lam [..., 2] -> q float32 [..., 2] and the unrounded float64"""
    sums, lam = np.asarray(sums), np.asarray(lam)
    q64 = np.zeros(lam.shape, np.float64)
    for idx in np.ndindex(*lam.shape[:-1]):
        q64[idx][0] = q_exact(sums[idx][N_EVAL], sums[idx][K_FW], lam[idx][0])
        q64[idx][1] = q_exact(sums[idx][N_EVAL], sums[idx][K_BW], lam[idx][1])
    return q64.astype(np.float32), q64


# ---- host-side verdicts ----------------------------------------------------------------------------------------------------------------

def verdict(n_eval, n_seen, q_fw, q_bw, min_variants, min_seen, q_min):
    if n_eval < min_variants:
        return NOT_EVALUABLE
    return DETECTED if n_seen >= min_seen and float(q_fw) >= q_min and float(q_bw) >= q_min else NOT_DETECTED


def excess(K, lam, D):
    if D <= 0:
        return 0.0
    x = (np.float64(int(K)) - np.float64(lam)) / np.float64(int(D))
    return float(x) if x > 0 else 0.0


def count_ge(obs_fw, obs_bw, ctl_q):
    """ctl_q float32 [R][2]"""
    obs = min(np.float32(obs_fw), np.float32(obs_bw))
    return int((np.minimum(ctl_q[:, 0], ctl_q[:, 1]) >= obs).sum()) if len(ctl_q) else 0


def empirical_p(n_ge, R):
    return float((np.float64(1.0) + np.float64(n_ge)) / (np.float64(R) + np.float64(1.0)))


def lod_reads(lam, q_min):
    """(K_min or 0, evaluations made)"""
    if not q_min <= 100.0 or not (0.0 <= lam < 2.0 ** 52):
        return 0, 0
    K = int(math.floor(lam)) + 1
    for i in range(LOD_MAX_EVALS):
        if float(np.float32(q_exact(1, K, lam))) >= q_min:
            return K, i + 1
        K += 1
    return 0, LOD_MAX_EVALS


def lod(lam_fw, lam_bw, D_fw, D_bw, q_min):
    if D_fw <= 0 or D_bw <= 0:
        return -1.0
    kf, kb = lod_reads(lam_fw, q_min)[0], lod_reads(lam_bw, q_min)[0]
    if kf <= 0 or kb <= 0:
        return -1.0
    a = (np.float64(kf) - np.float64(lam_fw)) / np.float64(int(D_fw))
    b = (np.float64(kb) - np.float64(lam_bw)) / np.float64(int(D_bw))
    return float(max(a, b))


# ---- the recorded grid (tests/golden/monitor/pool_grid.npz): python -m tests.monitor_model writes it -------------------------------------

GRID_LAMBDA = (1e-3, 1e-2, 0.1, 0.7, 1.0, 3.3, 10.0, 100.0, 1e3, 1e4, 1e5, 1e6)
CLAMP_LAMBDA = (0.5, 3.0, 20.0, 250.0, 1e4, 1e6)


def grid_cases():
    """(K int64, Lambda float64) of the grid: K at 0, 1, around Lambda and at Lambda + {1 .. 8} sqrt(Lambda), and the 1e-10 clamp approached
    from both sides"""
    out = []
    for lam in GRID_LAMBDA:
        fl, sd = int(math.floor(lam)), math.sqrt(lam)
        ks = {0, 1, 2, max(0, fl - 1), fl, fl + 1, fl + 2} | {int(lam + j * sd) for j in range(1, 9)} | {int(lam + j * sd) + 1 for j in range(1, 9)}
        ks |= {max(0, int(lam - j * sd)) for j in (1, 3)}
        out += [(k, lam) for k in sorted(ks)]
    for lam in CLAMP_LAMBDA:  # the clamp, both sides: the first K whose tail is below 1e-10, and its neighbours
        k = int(lam + 6.0 * math.sqrt(lam))
        while pois_tail(k, lam) >= mp.mpf(10) ** -10:
            k += 1
        out += [(kk, lam) for kk in (k - 2, k - 1, k, k + 1)]
    return np.array([c[0] for c in out], np.int64), np.array([c[1] for c in out], np.float64)


def random_cases(seed=24, n=20000):
    """(K int64, Lambda float64): Lambda log-uniform in [1e-3, 1e4], K from 0 to about Lambda + 8 sqrt(Lambda)"""
    rng = np.random.default_rng(seed)
    lam = np.exp(rng.uniform(math.log(1e-3), math.log(1e4), n))
    K = np.rint(lam * rng.uniform(0, 1.2, n) + np.sqrt(lam) * rng.uniform(0, 8, n) * (rng.random(n) < 0.5)).astype(np.int64) + rng.integers(0, 6, n)
    return K, lam


def write_golden(path):
    K, lam = grid_cases()
    rK, rlam = random_cases()
    K, lam = np.concatenate([K, rK]), np.concatenate([lam, rlam])
    q = np.array([q_exact(1, K[i], lam[i]) for i in range(len(K))], np.float64)
    np.savez_compressed(path, K=K, lam=lam, q=q, n_grid=len(K) - len(rK))
    return len(K)


if __name__ == "__main__":
    import os

    dst = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "monitor")
    os.makedirs(dst, exist_ok=True)
    print(write_golden(os.path.join(dst, "pool_grid.npz")), "cases")


# ---- the command line's three files as text (AmpliSolveVariantMonitoring) ---------------------------------------------------------------

VERDICT_NAMES = ("NOT_EVALUABLE", "NOT_DETECTED", "DETECTED")
HEAD = "sample\tlist\tN_eval\tN_seen\tK_fw\tK_bw\tD_fw\tD_bw\tLambda_fw\tLambda_bw\tQ_fw\tQ_bw\tExcess_fw\tExcess_bw\tVerdict"


def format_files(names, list_names, entries, P, own, sums, lam, q, n_ge, lods, params):
    """names: the samples in the command's order; own: [(sample index, list index)]; sums [S][L][6], lam [S][L][2], q float32 [S][L][2];
    n_ge and lods per own pair (a lod of -1 prints NA); params: coverage_cutoff, q_min, min_variants, min_seen, max_vaf_pm, controls,
    seed.  Returns the three texts and the verdicts [S][L]."""
    S, L = len(names), len(list_names)
    q_min, mv, ms = float(params["q_min"]), params["min_variants"], params["min_seen"]
    verdicts = np.array([[verdict(sums[s, l, N_EVAL], sums[s, l, N_SEEN], q[s, l, 0], q[s, l, 1], mv, ms, q_min) for l in range(L)] for s in range(S)])
    assigned = np.zeros((S, L), bool)
    for s, l in own:
        assigned[s, l] = True

    def row(s, l):
        c = sums[s, l]
        return (f"{names[s]}\t{list_names[l]}\t{c[0]}\t{c[1]}\t{c[2]}\t{c[3]}\t{c[4]}\t{c[5]}\t{lam[s, l, 0]:.6f}\t{lam[s, l, 1]:.6f}\t{float(q[s, l, 0]):.4f}\t"
                f"{float(q[s, l, 1]):.4f}\t{excess(c[K_FW], lam[s, l, 0], c[D_FW]):.6g}\t{excess(c[K_BW], lam[s, l, 1], c[D_BW]):.6g}\t{VERDICT_NAMES[verdicts[s, l]]}")

    matrix = HEAD + "\n" + "".join(row(s, l) + "\n" for s in range(S) for l in range(L))
    other = ((verdicts == DETECTED) & ~assigned).sum(axis=0)
    own_text = HEAD + "\tLoD\tN_ge\tControls\tEmpirical_p\tOther_detected\n"
    R = params["controls"]
    for k, (s, l) in enumerate(own):
        own_text += row(s, l) + f"\t{'NA' if lods[k] < 0 else format(lods[k], '.6g')}\t{n_ge[k]}\t{R}\t{empirical_p(n_ge[k], R):.6g}\t{other[l]}\n"
    ov = [sum(1 for s, l in own if verdicts[s, l] == v) for v in range(3)]
    summary = (f"samples={S}\nlists={L}\nentries={entries}\npositions={P}\nassigned_pairs={len(own)}\ncoverage_cutoff={params['coverage_cutoff']}\nq_min={q_min:g}\n"
               f"min_variants={mv}\nmin_seen={ms}\nmax_vaf_pm={params['max_vaf_pm']}\ncontrols={R}\nseed={params['seed']}\nmatrix_detected={(verdicts == DETECTED).sum()}\n"
               f"own_detected={ov[DETECTED]}\nown_not_detected={ov[NOT_DETECTED]}\nown_not_evaluable={ov[NOT_EVALUABLE]}\n"
               f"cross_detected={((verdicts == DETECTED) & ~assigned).sum()}\n")
    return {"Monitoring_Matrix.txt": matrix, "Monitoring_Own.txt": own_text, "Monitoring_Summary.txt": summary}, verdicts
