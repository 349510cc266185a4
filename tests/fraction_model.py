"""The definition of the tumour fraction per (sample, list) -- TEST INFRASTRUCTURE, and the text that
include/amplisolve_hip.h, csrc/ampli_math.h and DESIGN 26 restate.  How much of a patient's tumour is in this plasma sample, and within
what bounds: the score estimate of f and its Rao score interval.

  Lists.  Monitoring's CSR (tests/monitor_model.py: list_off uint32 [L + 1], list_cell uint32 [W], an entry c = 4 p + y) and list_w
    float32 [W], the weight a of every entry: the variant's allele fraction per unit of tumour fraction, for example its tissue VAF
    divided by the purity.  An entry with p >= P is none; a cell listed twice counts twice; offsets are cut to [0, W].
  Evaluated entry of a row.  Monitoring's rule -- the PRIMARY record is present, both strand depths >= coverage_cutoff, ref_code[p] in
    0..3 and y != it, both thresholds finite and >= 0, 1000 (k_fw + k_bw) <= max_vaf_pm (D_fw + D_bw), e == 0 replaced by
    float32(0.0010008) -- and a weight that is finite, > 0 and <= 1.  It gives two cells, fw then bw, each with k, d and e as doubles,
    a = double(w) and ad = a * d.  A cell is modelled as a Poisson count of mean d (e + f a).
  Score and information at f.  The operation sequence is part of the definition.  Per cell: r = e + f * a; g = a / r; U += g * k - ad;
    I += g * ad.  Lane j of 64 takes entries j, j + 64, ... ascending, fw before bw, into two accumulators that start at +0.0 (an entry
    that is not evaluated adds nothing); the 64 pairs are combined by x += x[lane ^ off] for off = 32, 16, 8, 4, 2, 1.
    T(f) = U * |U| / I.  N_EVAL: the evaluated entries; N_SEEN: those with k_fw + k_bw >= 1.
  Values.  N_EVAL == 0 or I(0) <= 0: all four are NA (-1).  Every bisection takes ITERS = 60 steps mid = 0.5 * (lo + hi) and gives
    0.5 * (lo + hi).
    F_HAT: 0 if U(0) <= 0; 1 if U(1) >= 0; else on [0, 1] with U(mid) > 0 ? lo = mid : hi = mid.
    F_LO:  0 if T(0) <= z2; else on [0, F_HAT] with T(mid) > z2 ? lo = mid : hi = mid.  T need not be monotone on [0, F_HAT] in
           contrived lists; the bisection's result is the definition.
    F_HI:  0 if F_HAT == 0 and -T(0) >= z2; 1 if -T(1) < z2; else on [F_HAT, 1] with -T(mid) < z2 ? lo = mid : hi = mid.
    T0 = T(0).
  Verdicts.  NOT_EVALUABLE if N_EVAL < min_variants (or the values are NA); QUANTIFIED if F_LO > 0; else BELOW, and F_HI is the
    reportable upper bound.  Change from draw A to draw B of one list: NOT_EVALUABLE if either draw is; RISING if F_LO_B > F_HI_A;
    FALLING if F_HI_B < F_LO_A; else STABLE; the ratio is F_HAT_B / F_HAT_A, NA at a zero denominator.

Every sum here is written with the explicit 64-lane order (never np.sum); the arrays carry a leading batch axis so that many (row, list)
pairs -- or the replicates of a simulation -- run the same operations side by side, each exactly as it would alone."""
from __future__ import annotations

import numpy as np

from tests.monitor_model import ABSENT, E0, LANES, cut, thr_ok

F_HAT, F_LO, F_HI, T0, VALS = 0, 1, 2, 3, 4
N_EVAL, N_SEEN, COUNTS = 0, 1, 2
NA = -1.0
ITERS = 60
Z2 = {"0.90": 2.705543, "0.95": 3.841459, "0.99": 6.634897}
Z2_95 = Z2["0.95"]
NOT_EVALUABLE, BELOW, QUANTIFIED = 0, 1, 2
CHANGE_NOT_EVALUABLE, STABLE, RISING, FALLING = 0, 1, 2, 3


def weight_ok(w):
    w = np.float32(w)
    return bool(np.isfinite(w) and 0 < w <= 1)


def butterfly(acc):
    """[B, 64] accumulators combined per row: x += x[lane ^ off] for off = 32, 16, 8, 4, 2, 1 -> [B]"""
    acc = np.array(acc, np.float64)
    assert acc.shape[-1] == 64
    for off in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[..., LANES ^ off]
    return acc[..., 0]


class Cells:
    """the cells of B (row, list) pairs in the order a wave adds them: step s = 2 * round + strand, lane j -- k, ad, a, e float64
    [B, S, 64] and ok bool [B, S, 64] (an entry that is not evaluated: False on both of its steps)"""

    def __init__(self, k, ad, a, e, ok):
        self.k, self.ad, self.a, self.e, self.ok = (np.ascontiguousarray(x) for x in (k, ad, a, e, ok))
        assert self.k.shape == self.ad.shape == self.a.shape == self.e.shape == self.ok.shape and self.k.shape[-1] == 64

    @property
    def n_eval(self):
        return self.ok[:, 0::2].sum(axis=(1, 2))  # an integer count: order-free


def sums_at(c: Cells, f):
    """U(f), I(f) float64 [B] for f float64 [B]"""
    f = np.asarray(f, np.float64)
    B, S, _ = c.k.shape
    u, i = np.zeros((B, 64)), np.zeros((B, 64))
    with np.errstate(divide="ignore", invalid="ignore"):
        for s in range(S):
            r = c.e[:, s] + f[:, None] * c.a[:, s]
            g = c.a[:, s] / r
            u = np.where(c.ok[:, s], u + (g * c.k[:, s] - c.ad[:, s]), u)
            i = np.where(c.ok[:, s], i + g * c.ad[:, s], i)
    return butterfly(u), butterfly(i)


def T_of(U, I):
    with np.errstate(divide="ignore", invalid="ignore"):
        return U * np.abs(U) / I


def _bisect(c, lo, hi, go_up):
    """ITERS steps for every pair side by side; go_up(U, I) -> bool [B]: lo = mid, else hi = mid"""
    lo, hi = np.array(lo, np.float64), np.array(hi, np.float64)
    for _ in range(ITERS):
        mid = 0.5 * (lo + hi)
        up = go_up(*sums_at(c, mid))
        lo, hi = np.where(up, mid, lo), np.where(up, hi, mid)
    return 0.5 * (lo + hi)


def solve(c: Cells, z2=Z2_95):
    """-> float64 [B, 4]: F_HAT, F_LO, F_HI, T0.  A pair whose first rule decides runs the bisection too and drops its result: the
    value is the same as if it had not."""
    B = c.k.shape[0]
    zero, one = np.zeros(B), np.ones(B)
    U0, I0 = sums_at(c, zero)
    U1, I1 = sums_at(c, one)
    t0, t1 = T_of(U0, I0), T_of(U1, I1)
    fh = _bisect(c, zero, one, lambda U, I: U > 0)
    fh = np.where(U0 <= 0, 0.0, np.where(U1 >= 0, 1.0, fh))
    fl = _bisect(c, zero, fh, lambda U, I: T_of(U, I) > z2)
    fl = np.where(t0 > z2, fl, 0.0)
    fu = _bisect(c, fh, one, lambda U, I: -T_of(U, I) < z2)
    fu = np.where((fh == 0) & (-t0 >= z2), 0.0, np.where(-t1 < z2, 1.0, fu))
    out = np.stack([fh, fl, fu, t0], axis=1)
    out[(c.n_eval <= 0) | ~(I0 > 0)] = NA
    return out


def list_cells(recs, P, thr, ref_code, cell, w, cov, max_vaf_pm):
    """one list over the rows recs int [n][>= P][8]: cell the list's entries (4 p + y), w its weights -> Cells with B = n, and the
    counts int64 [n, 2]"""
    thr = np.asarray(thr, np.float32).reshape(2, 4, P)
    n, m = len(recs), len(cell)
    R = max(1, -(-m // 64))
    k, ad, a, e = (np.zeros((n, 2 * R, 64)) for _ in range(4))
    ok = np.zeros((n, 2 * R, 64), bool)
    count = np.zeros((n, COUNTS), np.int64)
    for i in range(m):
        p, y = int(cell[i]) >> 2, int(cell[i]) & 3
        if p >= P or ref_code[p] > 3 or y == ref_code[p]:
            continue
        ef, eb = thr[0, y, p], thr[1, y, p]
        if not (thr_ok(ef) and thr_ok(eb) and weight_ok(w[i])):
            continue
        aw = np.float64(np.float32(w[i]))
        rnd, lane = i >> 6, i & 63
        for s in range(n):
            r = [int(x) for x in recs[s][p]]
            if r[0] == ABSENT:
                continue
            FW, BW, kf, kb = sum(r[:4]), sum(r[4:]), r[y], r[4 + y]
            if FW < cov or BW < cov or 1000 * (kf + kb) > max_vaf_pm * (FW + BW):
                continue
            count[s, N_EVAL] += 1
            count[s, N_SEEN] += kf + kb >= 1
            for st, (kk, dd, ee) in enumerate(((kf, FW, ef), (kb, BW, eb))):
                j = 2 * rnd + st
                ok[s, j, lane] = True
                k[s, j, lane] = np.float64(kk)
                ad[s, j, lane] = aw * np.float64(dd)
                a[s, j, lane] = aw
                e[s, j, lane] = np.float64(E0 if ee == 0 else ee)
    return Cells(k, ad, a, e, ok), count


def fraction_model(recs, P, thr, ref_code, list_off, list_cell, list_w, cov=100, max_vaf_pm=1000, z2=Z2_95):
    """recs int32 [n][>= P][8] -> est float64 [n][L][4], count int64 [n][L][2]"""
    n, L, W = len(recs), len(list_off) - 1, len(list_cell)
    est, count = np.zeros((n, L, VALS)), np.zeros((n, L, COUNTS), np.int64)
    for l in range(L):
        off, end = cut(list_off, l, W)
        c, count[:, l] = list_cells(recs, P, thr, ref_code, list_cell[off:end], list_w[off:end], cov, max_vaf_pm)
        est[:, l] = solve(c, z2)
    return est, count


def cells_from_counts(k, d, e, a):
    """Cells of B lists given apart, for the tests of the arithmetic alone: k, d int [B][m][2] (fw, bw), e float32 [B][m][2], a float32
    [B][m]; every entry is evaluated"""
    k, d, e, a = np.asarray(k), np.asarray(d), np.asarray(e, np.float32), np.asarray(a, np.float32)
    B, m = a.shape
    R = max(1, -(-m // 64))
    shape = (B, R, 64, 2)
    K, AD, A, E = (np.zeros(shape) for _ in range(4))
    ok = np.zeros(shape, bool)
    idx = np.arange(m)
    rnd, lane = idx >> 6, idx & 63
    aw = a.astype(np.float64)
    K[:, rnd, lane] = k.astype(np.float64)
    AD[:, rnd, lane] = aw[:, :, None] * d.astype(np.float64)
    A[:, rnd, lane] = aw[:, :, None]
    E[:, rnd, lane] = np.where(e == 0, E0, e).astype(np.float64)
    ok[:, rnd, lane] = True

    def steps(x):  # [B, R, 64, 2] -> [B, 2 R, 64]
        return x.transpose(0, 1, 3, 2).reshape(B, 2 * R, 64)

    return Cells(steps(K), steps(AD), steps(A), steps(E), steps(ok))


# ---- host-side verdicts ----------------------------------------------------------------------------------------------------------------

def verdict(n_eval, f_hat, f_lo, min_variants):
    if n_eval < min_variants or f_hat < 0:
        return NOT_EVALUABLE
    return QUANTIFIED if f_lo > 0 else BELOW


def change(verdict_a, a, verdict_b, b):
    """-> (code, ratio)"""
    if verdict_a == NOT_EVALUABLE or verdict_b == NOT_EVALUABLE:
        return CHANGE_NOT_EVALUABLE, NA
    ratio = float(np.float64(b[F_HAT]) / np.float64(a[F_HAT])) if a[F_HAT] > 0 else NA
    if b[F_LO] > a[F_HI]:
        return RISING, ratio
    if b[F_HI] < a[F_LO]:
        return FALLING, ratio
    return STABLE, ratio


# ---- the 50-digit reference and the recorded grid (tests/golden/fraction/grid.npz): python -m tests.fraction_model writes it ---------------

DPS = 50


def exact_roots(k, d, e, a, z2=Z2_95):
    """One list in mpmath at DPS digits: the roots of U = 0, T = z2 on [0, f_hat] and T = -z2 on [f_hat, 1] by bisection to 1e-40, None
    where the model's first rules decide instead (U(0) <= 0, U(1) >= 0, T(0) <= z2, -T(1) < z2).  k, d [m][2], e [m][2], a [m]: the
    float32 values taken exactly."""
    import mpmath as mp

    with mp.workdps(DPS):
        kk = [mp.mpf(int(x)) for x in np.asarray(k).ravel()]
        dd = [mp.mpf(int(x)) for x in np.asarray(d).ravel()]
        ee = [mp.mpf(float(x)) for x in np.asarray(e, np.float32).ravel()]
        aa = [mp.mpf(float(x)) for x in np.repeat(np.asarray(a, np.float32), 2)]

        def UI(f):
            U = I = mp.mpf(0)
            for kx, dx, ex, ax in zip(kk, dd, ee, aa):
                g = ax / (ex + f * ax)
                U += g * kx - ax * dx
                I += g * ax * dx
            return U, I

        def T(f):
            U, I = UI(f)
            return U * abs(U) / I

        def root(fn, lo, hi):  # fn(lo) > 0 >= fn(hi)
            lo, hi = mp.mpf(lo), mp.mpf(hi)
            while hi - lo > mp.mpf(10) ** -40:
                mid = (lo + hi) / 2
                if fn(mid) > 0:
                    lo = mid
                else:
                    hi = mid
            return (lo + hi) / 2

        z = mp.mpf(z2)
        if UI(0)[0] <= 0:
            fh = None
        elif UI(1)[0] >= 0:
            fh = None
        else:
            fh = root(lambda f: UI(f)[0], 0, 1)
        fl = root(lambda f: T(f) - z, 0, fh) if fh is not None and T(0) > z else None
        fu = root(lambda f: z + T(f), fh, 1) if fh is not None and -T(1) >= z else None
        return tuple(None if x is None else float(x) for x in (fh, fl, fu))


GRID_M = (1, 2, 3, 7, 14, 40, 63, 64, 65, 130, 300)
GRID_DEPTH = (1e2, 1e3, 1e4, 1e5, 1e6, 1e7)
GRID_F = (1e-5, 1e-4, 1e-3, 1e-2, 0.1, 0.5)


def grid_lists(seed=26):
    """the grid as a list of (k [m][2], d [m][2], e float32 [m][2], a float32 [m]): every (m, depth, f), counts Poisson at d (e + f a)"""
    rng = np.random.default_rng(seed)
    out = []
    for m in GRID_M:
        for depth in GRID_DEPTH:
            for f in GRID_F:
                d = rng.integers(int(0.8 * depth), int(1.2 * depth) + 1, (m, 2))
                e = rng.uniform(0.0003, 0.001, (m, 2)).astype(np.float32)
                a = rng.uniform(0.2, 0.6, m).astype(np.float32)
                k = rng.poisson(d * (e.astype(np.float64) + f * a.astype(np.float64)[:, None]))
                out.append((k.astype(np.int64), d.astype(np.int64), e, a))
    return out


def write_golden(path):
    lists = grid_lists()
    roots = np.full((len(lists), 3), np.nan)
    for i, (k, d, e, a) in enumerate(lists):
        roots[i] = [np.nan if x is None else x for x in exact_roots(k, d, e, a)]
    m = np.array([len(x[3]) for x in lists], np.int64)
    np.savez_compressed(path, m=m, k=np.concatenate([x[0] for x in lists]), d=np.concatenate([x[1] for x in lists]),
                        e=np.concatenate([x[2] for x in lists]), a=np.concatenate([x[3] for x in lists]), roots=roots)
    return len(lists)


def read_golden(path):
    """-> [(k, d, e, a)], roots float64 [n][3] (NaN where a first rule decides)"""
    g = np.load(path)
    off = np.concatenate([[0], np.cumsum(g["m"])])
    return [(g["k"][lo:hi], g["d"][lo:hi], g["e"][lo:hi], g["a"][lo:hi]) for lo, hi in zip(off[:-1], off[1:])], g["roots"]


if __name__ == "__main__":
    import os

    dst = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fraction")
    os.makedirs(dst, exist_ok=True)
    print(write_golden(os.path.join(dst, "grid.npz")), "lists")


# ---- the command line's four files as text (AmpliSolveTumourFraction) --------------------------------------------------------------------

VERDICT_NAMES = ("NOT_EVALUABLE", "BELOW", "QUANTIFIED")
CHANGE_NAMES = ("NOT_EVALUABLE", "STABLE", "RISING", "FALLING")
HEAD = "sample\tlist\tN_eval\tN_seen\tF_hat\tF_lo\tF_hi\tT0\tVerdict"
CHANGE_HEAD = "list\tsample_a\tsample_b\tF_hat_a\tF_lo_a\tF_hi_a\tF_hat_b\tF_lo_b\tF_hi_b\tRatio\tChange"


def _num(x):
    return "NA" if x == NA else format(float(x), ".6g")


def format_files(names, list_names, entries, P, own, est, count, params):
    """names: the samples in the command's order; own: [(sample index, list index)] in the order of the assignments; est [S][L][4], count
    [S][L][2]; params: coverage_cutoff, min_variants, max_vaf_pm, confidence (the text's key of Z2).  Returns the four texts, the
    verdicts [S][L] and the changes [(own index of draw B, code, ratio)]."""
    S, L = len(names), len(list_names)
    mv = params["min_variants"]
    verdicts = np.array([[verdict(count[s, l, N_EVAL], est[s, l, F_HAT], est[s, l, F_LO], mv) for l in range(L)] for s in range(S)])

    def row(s, l):
        v = est[s, l]
        t0 = "NA" if v[F_HAT] == NA else format(float(v[T0]), ".6g")
        return f"{names[s]}\t{list_names[l]}\t{count[s, l, 0]}\t{count[s, l, 1]}\t{_num(v[F_HAT])}\t{_num(v[F_LO])}\t{_num(v[F_HI])}\t{t0}\t{VERDICT_NAMES[verdicts[s, l]]}"

    matrix = HEAD + "\n" + "".join(row(s, l) + "\n" for s in range(S) for l in range(L))
    own_text = HEAD + "\n" + "".join(row(s, l) + "\n" for s, l in own)
    change_text, changes = CHANGE_HEAD + "\n", []
    for k in range(1, len(own)):
        (sa, la), (sb, lb) = own[k - 1], own[k]
        if la != lb:
            continue
        code, ratio = change(verdicts[sa, lb], est[sa, lb], verdicts[sb, lb], est[sb, lb])
        changes.append((k, code, ratio))
        a, b = est[sa, lb], est[sb, lb]
        change_text += (f"{list_names[lb]}\t{names[sa]}\t{names[sb]}\t{_num(a[F_HAT])}\t{_num(a[F_LO])}\t{_num(a[F_HI])}\t{_num(b[F_HAT])}\t{_num(b[F_LO])}\t"
                        f"{_num(b[F_HI])}\t{_num(ratio)}\t{CHANGE_NAMES[code]}\n")
    ov = [sum(1 for s, l in own if verdicts[s, l] == v) for v in range(3)]
    nc = [sum(1 for _, c, _ in changes if c == v) for v in range(4)]
    summary = (f"samples={S}\nlists={L}\nentries={entries}\npositions={P}\nassigned_pairs={len(own)}\ncoverage_cutoff={params['coverage_cutoff']}\n"
               f"min_variants={mv}\nmax_vaf_pm={params['max_vaf_pm']}\nconfidence={float(params['confidence']):.2f}\nz2={Z2[params['confidence']]:g}\n"
               f"matrix_quantified={(verdicts == QUANTIFIED).sum()}\nown_quantified={ov[QUANTIFIED]}\nown_below={ov[BELOW]}\nown_not_evaluable={ov[NOT_EVALUABLE]}\n"
               f"changes={len(changes)}\nrising={nc[RISING]}\nfalling={nc[FALLING]}\nstable={nc[STABLE]}\nchange_not_evaluable={nc[CHANGE_NOT_EVALUABLE]}\n")
    return {"Fraction_Matrix.txt": matrix, "Fraction_Own.txt": own_text, "Fraction_Change.txt": change_text, "Fraction_Summary.txt": summary}, verdicts, changes
