"""Overdispersion-aware calling, the definition -- TEST INFRASTRUCTURE.

The fit.  A cell is (strand, base, position); its qualifying records are dispersion's (tests/dispersion_model.py: the ones cnt counts).
With n, K = sum k_i, D = sum d_i, S2 = sum d_i^2 over them and X2 Pearson's statistic of dispersion:

    omega = (X2 - (n - 1)) D / (K (D - S2 / D))   where the cell's status carries HIGH and D - S2 / D > 0, and the quotient is above 0
    omega = 0                                      everywhere else

S2 is a Python integer; omega is a Fraction of the double X2 it is given (the X2 the code under test was given too).

The score.  k reads of d on a strand, e the table's float threshold, omega a double:

    NA (-1)  for a negative, NaN or infinite omega; else -888 for e == -1; else 0 for k == 0; else, e == 0 replaced by float32(0.0010008),
    m = double(d) * double(e) (one double product), p = P[X >= k] for X negative binomial of mean m and variance m + omega m^2
    (omega = 0: Poisson), Q = 0 for p >= 1, else float32(-10 log10(max(p, 1e-10))).

The tail is summed in mpmath at 50 digits from a start term formed with loggamma: the complement 1 - sum_{j < k} pmf(j) where k terms
are the fewer (at 50 digits the subtraction costs nothing down to p = 1e-30), else from k upwards until what is left is below 1e-30 of
the sum (every later ratio is below max(the next ratio, m omega / (1 + m omega)) < 1).  scipy's nbinom.sf is 5e-8 off at omega = 1e-9
and is used as a cross-check only (tests/test_overdispersion_model.py).
"""
from __future__ import annotations

import functools
import math
from fractions import Fraction

import mpmath as mp
import numpy as np

from tests.dispersion_model import ABSENT, HIGH, qualifying

NA = np.float32(-1.0)
DPS = 50


def s2_model(recs, P, cov, E=0, ext_pos=None):
    """S2 as Python integers, object array [2][4][P]; recs int32 [S][P+E][8]"""
    recs = np.ascontiguousarray(recs, np.int64)
    S, R = recs.shape[0], recs.shape[1]
    assert R == P + E
    pos = np.arange(R)
    if E:
        pos[P:] = np.asarray(ext_pos, np.int64)
    q = qualifying(recs, cov)
    present = recs[:, :, 0] != ABSENT
    out = np.zeros((2, 4, P), object)
    for st in range(2):
        d = np.where(present, recs[:, :, st * 4:st * 4 + 4].sum(axis=2), 0).astype(object)
        d2 = d * d
        for nt in range(4):
            ss, rr = np.nonzero(q[:, :, nt])
            np.add.at(out[st, nt], pos[rr], d2[ss, rr])
    return out


def omega_exact(status, n, K, D, x2, S2):
    """one cell: a Fraction.  n, K, D, S2 integers, x2 the double X2"""
    if not (int(status) & HIGH):
        return Fraction(0)
    n, K, D, S2 = int(n), int(K), int(D), int(S2)
    den = D - Fraction(S2, D)
    if den <= 0:
        return Fraction(0)
    w = (Fraction(float(x2)) - (n - 1)) * D / (K * den)
    return w if w > 0 else Fraction(0)


def omega_bound(w, D, S2):
    """what five roundings and the subtraction D - S2 / D may cost: 16 * 2^-53 * omega * (2 + S2 / (D^2 - S2))"""
    D, S2 = int(D), int(S2)
    return float(16 * Fraction(1, 2 ** 53) * w * (2 + Fraction(S2, D * D - S2))) if w > 0 else 0.0


def omega_model(status, n, K, D, x2, S2):
    """planes [2][4][P] (n [4][P]) -> omega float64 and the bound float64"""
    w = np.zeros(status.shape, np.float64)
    b = np.zeros(status.shape, np.float64)
    for st, nt, p in zip(*np.nonzero(status & HIGH)):
        e = omega_exact(status[st, nt, p], n[nt, p], K[st, nt, p], D[st, nt, p], x2[st, nt, p], S2[st, nt, p])
        w[st, nt, p] = float(e)
        b[st, nt, p] = omega_bound(e, D[st, nt, p], S2[st, nt, p])
    return w, b


@functools.lru_cache(maxsize=None)
def nb_tail(k, m, w):
    """P[X >= k] as an mpf; k an int, m and w doubles (taken exactly)"""
    k = int(k)
    # loggamma(j + 1 / omega) - loggamma(1 / omega) cancels log10(1 / omega) digits
    with mp.workdps(DPS + (int(-math.log10(w)) + 5 if 0 < w < 1 else 0)):
        if k <= 0:
            return mp.mpf(1)
        if not m > 0:
            return mp.mpf(0)
        m, w = mp.mpf(m), mp.mpf(w)
        a = 1 + m * w
        qq, lim = m / a, m * w / a

        def logpmf(j):
            if w == 0:
                return j * mp.log(m) - m - mp.loggamma(j + 1)
            s = 1 / w
            return mp.loggamma(j + s) - mp.loggamma(j + 1) - mp.loggamma(s) - s * mp.log1p(m * w) + j * mp.log(lim)

        cost_up = 90 * float(a) + 14 * math.sqrt(float(m + w * m * m)) + 50 if k > m else math.inf
        if k <= cost_up:
            t = mp.exp(logpmf(0))
            sm = t
            for j in range(k - 1):
                t = t * (1 + j * w) / (j + 1) * qq
                sm += t
            return 1 - sm if sm < 1 else mp.mpf(0)
        t = mp.exp(logpmf(k))
        sm, j, eps = t, k, mp.mpf(10) ** -30
        while True:
            r = (1 + j * w) / (j + 1) * qq
            if t * r < eps * sm * (1 - max(r, lim)):
                return sm
            t *= r
            sm += t
            j += 1


E0 = np.float32(0.0010008)


def nb_q_exact(k, d, e, w):
    """Q before it is rounded to a float: an mpf, or the exact -1 / -888 / 0"""
    w = float(w)
    if not (w >= 0.0) or math.isinf(w):
        return mp.mpf(-1)
    e = np.float32(e)
    if e == np.float32(-1):
        return mp.mpf(-888)
    if int(k) == 0:
        return mp.mpf(0)
    if e == 0:
        e = E0
    p = nb_tail(int(k), float(d) * float(e), w)
    with mp.workdps(DPS):
        if p >= 1:
            return mp.mpf(0)
        return -10 * mp.log10(max(p, mp.mpf(10) ** -10))


def nb_q(k, d, e, w):
    return np.float32(float(nb_q_exact(k, d, e, w)))


def score_model(trecs, P, thr, omega, ref_code, cutoff):
    """trecs int32 [n_t][>= P][8] (primary slots), thr float32 [2][4][P], omega float64 [2][4][P] or None -> q float32 [n_t][P][4][2]
    and float64 of the same shape (the unrounded Q)"""
    trecs = np.asarray(trecs, np.int64)[:, :P]
    thr = np.asarray(thr, np.float32).reshape(2, 4, P)
    n_t = trecs.shape[0]
    q = np.full((n_t, P, 4, 2), NA, np.float32)
    q64 = np.full((n_t, P, 4, 2), -1.0, np.float64)
    for t in range(n_t):
        for p in range(P):
            r = trecs[t, p]
            if r[0] == ABSENT or ref_code[p] > 3:
                continue
            D = (int(r[0:4].sum()), int(r[4:8].sum()))
            if D[0] < cutoff or D[1] < cutoff:
                continue
            for b in range(4):
                if b == ref_code[p]:
                    continue
                for st in range(2):
                    v = nb_q_exact(int(r[st * 4 + b]), D[st], thr[st, b, p], 0.0 if omega is None else omega[st, b, p])
                    q64[t, p, b, st] = float(v)
                    q[t, p, b, st] = np.float32(float(v))
    return q, q64


def decisions(q, q_min):
    """[n_t][P][4]: 1 where the cell is evaluated and Q >= q_min on both strands"""
    return ((q[..., 0] >= q_min) & (q[..., 1] >= q_min)).astype(np.uint8)


def format_files(names, n_normals, positions, bases, ref_code, trecs, q0, q, omega, disp, params):
    """the command line's four files as text.  names: the tumours'; positions [(chrom, coordinate)]; bases: the reference base as the
    panel spells it; trecs int32 [T][>= P][8]; q0, q float32 [T][P][4][2]; omega float64 [2][4][P]; disp: the dispersion model's planes
    (n, K, D, x2, z); params: C_value, coverage_cutoff, calling_cutoff, z_cutoff, q_min"""
    P, q_min = len(positions), float(params["q_min"])
    cells = "chrom\tposition\tref\tbase\tstrand\tN\tAltReads\tDepth\tX2\tZ\tOmega\n"
    fitted = 0
    for p in range(P):
        for nt in range(4):
            for st in range(2):
                if not omega[st, nt, p] > 0:
                    continue
                fitted += 1
                cells += (f"{positions[p][0]}\t{positions[p][1]}\t{bases[p]}\t{'ACGT'[nt]}\t{'+-'[st]}\t{disp['n'][nt, p]}\t{int(disp['K'][st, nt, p])}\t"
                          f"{int(disp['D'][st, nt, p])}\t{disp['x2'][st, nt, p]:.6f}\t{disp['z'][st, nt, p]:.4f}\t{omega[st, nt, p]:.6g}\n")
    calls = "sample\tchrom\tposition\tsubstitution\tXfw\tXrs\tFW\tBW\tQ0_fw\tQ0_rs\tOmega_fw\tOmega_rs\tQ_fw\tQ_rs\tVerdict\n"
    samples = "sample\tEvaluated\tPoisson\tKept\tDropped\n"
    tot = [0, 0, 0]
    for t, name in enumerate(names):
        ev = po = ke = 0
        for p in range(P):
            r = trecs[t, p].astype(np.int64)
            for y in range(4):
                if q0[t, p, y, 0] == NA:
                    continue
                ev += 1
                if not (q0[t, p, y, 0] >= q_min and q0[t, p, y, 1] >= q_min):
                    continue
                po += 1
                kept = bool(q[t, p, y, 0] >= q_min and q[t, p, y, 1] >= q_min)
                ke += kept
                calls += (f"{name}\t{positions[p][0]}\t{positions[p][1]}\t{'ACGT'[ref_code[p]]}->{'ACGT'[y]}\t{r[y]}\t{r[4 + y]}\t{r[:4].sum()}\t{r[4:].sum()}\t"
                          f"{q0[t, p, y, 0]:.4f}\t{q0[t, p, y, 1]:.4f}\t{omega[0, y, p]:.6g}\t{omega[1, y, p]:.6g}\t{q[t, p, y, 0]:.4f}\t{q[t, p, y, 1]:.4f}\t"
                          f"{'KEPT' if kept else 'DROPPED'}\n")
        samples += f"{name}\t{ev}\t{po}\t{ke}\t{po - ke}\n"
        tot = [tot[0] + ev, tot[1] + po, tot[2] + ke]
    summary = (f"normals={n_normals}\ntumours={len(names)}\npositions={P}\nC_value={params['C_value']:g}\ncoverage_cutoff={params['coverage_cutoff']}\n"
               f"calling_cutoff={params['calling_cutoff']}\nz_cutoff={params['z_cutoff']:g}\nq_min={q_min:g}\ncells_fitted={fitted}\nevaluated={tot[0]}\n"
               f"poisson={tot[1]}\nkept={tot[2]}\ndropped={tot[1] - tot[2]}\n")
    return {"Overdispersed_Calls.txt": calls, "Overdispersed_Cells.txt": cells, "Overdispersed_Samples.txt": samples, "Overdispersed_Summary.txt": summary}


# ---- the recorded grid (tests/golden/overdispersion/nb_grid.npz): python -m tests.overdispersion_model writes it ----------------------

GRID_M = (1e-3, 1e-2, 0.1, 0.7, 1.0, 3.3, 10.0, 100.0, 1e3, 1e4)
GRID_W = (0.0, 1e-300, 1e-12, 1e-8, 1e-6, 1e-4, 1e-2, 0.1, 0.5, 1.0, 1.5, 10.0, 100.0, 1e4)
D_MAX = 2 ** 31 - 1


def _de(m, d):
    """a float32 e with double(d) * double(e) next to m"""
    return np.float32(m / d)


def grid_cases(seed=19, n_random=20000):
    """(k, d, e, omega) of the grid, the special values, the clamp and n_random random quadruples; int32, int32, float32, float64"""
    rng = np.random.default_rng(seed)
    out = []
    for m in GRID_M:
        for d in (max(100, int(4 * m) + 7), 1000003, D_MAX):
            e = _de(m, d)
            mm = float(d) * float(e)
            for w in GRID_W:
                ks = {0, 1, 2, max(0, int(mm) - 1), int(mm), int(mm) + 1, int(mm) + 2, int(10 * mm), int(10 * mm) + 1}
                out += [(k, d, e, w) for k in sorted(ks)]
    for w in (0.0, 1.5):  # e == -1 and e == 0, at k == 0 too
        out += [(k, d, e, w) for k in (0, 1, 5) for d in (100, 5000, D_MAX) for e in (np.float32(-1), np.float32(0))]
    for m, w in ((0.5, 0.0), (3.0, 0.0), (20.0, 0.0), (0.5, 0.3), (3.0, 1.5), (20.0, 0.05), (2.0, 1e-8), (1.0, 10.0)):  # the clamp, both sides
        d = 20011
        e = _de(m, d)
        k = int(m) + 1
        while nb_tail(k, float(d) * float(e), w) >= mp.mpf(10) ** -10 and k < 4000:
            k += 1
        out += [(kk, d, e, w) for kk in (k - 2, k - 1, k, k + 1)]
    d = np.exp(rng.uniform(math.log(100), math.log(D_MAX), n_random)).astype(np.int64)
    m = np.exp(rng.uniform(math.log(1e-3), math.log(100.0), n_random))
    w = np.where(rng.random(n_random) < 0.2, 0.0, np.exp(rng.uniform(math.log(1e-8), math.log(1e4), n_random)))
    k = np.rint(m * rng.uniform(0, 3, n_random)).astype(np.int64) + rng.integers(0, 6, n_random)
    out += [(int(k[i]), int(d[i]), _de(m[i], d[i]), float(w[i])) for i in range(n_random)]
    return (np.array([c[0] for c in out], np.int32), np.array([c[1] for c in out], np.int32), np.array([c[2] for c in out], np.float32),
            np.array([c[3] for c in out], np.float64))


def write_golden(path):
    k, d, e, w = grid_cases()
    q = np.array([float(nb_q_exact(k[i], d[i], e[i], w[i])) for i in range(len(k))], np.float64)
    np.savez_compressed(path, k=k, d=d, e=e, omega=w, q=q)
    return len(k)


if __name__ == "__main__":
    import os

    dst = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "overdispersion")
    os.makedirs(dst, exist_ok=True)
    print(write_golden(os.path.join(dst, "nb_grid.npz")), "cases")
