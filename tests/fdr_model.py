"""The definition of false-discovery control in numpy, float64: the Benjamini-Hochberg adjusted score of every cell of a
score plane s [rows, P, 4, 2] (row, position, base, strand), each row on its own.  The public header, the host library
(ampli_host_fdr_rows) and the kernels (csrc/ampli_fdr.hip) state the same text.

Cell key, with s_f and s_b the two strand scores:
  two_sided == 0:  TESTED iff 0 <= s_f <= 100 and 0 <= s_b <= 100; a = min(s_f, s_b), sign +.
  two_sided == 1:  TESTED iff -100 <= s_f <= 100 and -100 <= s_b <= 100; both > 0: a = min, sign +; both < 0: a = min(|s_f|, |s_b|),
                   sign -; otherwise a = 0.
  Everything else is untested: NaN, +-inf, any sentinel, anything beyond +-100.  A zero of either sign is a = 0.
Adjustment: m = the tested cells of the row (a = 0 included); for a tested cell with a > 0
  R = #{tested j : a_j >= a},   B = a - 10 log10(m / R) - (two_sided ? 10 log10 2 : 0),   A = max(0, max{B_j : 0 < a_j <= a}).
Output: sign * A; +0 where a = 0 or A = 0; NA (-999) where untested; m per row; R per cell (0 where untested or a = 0).
"""
import numpy as np

NA = -999.0
UNTESTED, ZERO, PLUS, MINUS = 0, 1, 2, 3


def keys(s, two_sided):
    """(a float64 [..., 4] magnitude, cls int [..., 4]) of a plane [..., 4, 2] of float32 scores."""
    s = np.asarray(s, np.float32).astype(np.float64)
    f, b = s[..., 0], s[..., 1]
    lo = -100.0 if two_sided else 0.0
    with np.errstate(invalid="ignore"):
        tested = (f >= lo) & (f <= 100.0) & (b >= lo) & (b <= 100.0)
        plus = tested & (f > 0) & (b > 0)
        minus = tested & (f < 0) & (b < 0)
    cls = np.where(plus, PLUS, np.where(minus, MINUS, np.where(tested, ZERO, UNTESTED)))
    a = np.where(plus, np.minimum(f, b), np.where(minus, np.minimum(-f, -b), 0.0))
    return np.where(tested, a, 0.0), cls


def adjust_row(a, cls, two_sided):
    """One row: a, cls flat arrays.  Returns (signed A float64 with NA, m, R int64)."""
    a, cls = np.asarray(a, np.float64).ravel(), np.asarray(cls).ravel()
    m = int((cls != UNTESTED).sum())
    out = np.where(cls == UNTESTED, NA, 0.0)
    R = np.zeros(a.shape, np.int64)
    pos = np.flatnonzero(cls >= PLUS)
    if pos.size:
        v = a[pos]
        u, inv, cnt = np.unique(v, return_inverse=True, return_counts=True)  # ascending
        rank_u = cnt[::-1].cumsum()[::-1]  # cells with a key >= u: every positive key is tested
        B = u - 10.0 * np.log10(m / rank_u) - (10.0 * np.log10(2.0) if two_sided else 0.0)
        A_u = np.maximum(0.0, np.maximum.accumulate(B))
        A = A_u[inv]
        out[pos] = np.where(cls[pos] == MINUS, -A, A) + 0.0  # -0 + 0 = +0
        R[pos] = rank_u[inv]
    return out, m, R


def adjust(s, two_sided):
    """The whole plane s [rows, P, 4, 2]: (A float64 [rows, P, 4], m int64 [rows], R int64 [rows, P, 4])."""
    s = np.asarray(s, np.float32)
    rows, P = s.shape[0], s.shape[1]
    a, cls = keys(s, two_sided)
    A, m, R = np.empty((rows, P, 4)), np.empty((rows,), np.int64), np.empty((rows, P, 4), np.int64)
    for r in range(rows):
        o, m[r], rr = adjust_row(a[r], cls[r], two_sided)
        A[r], R[r] = o.reshape(P, 4), rr.reshape(P, 4)
    return A, m, R


def adjust_row_literal(a, cls, two_sided):
    """The definition word for word, O(m^2): for small rows in the tests."""
    a, cls = np.asarray(a, np.float64).ravel(), np.asarray(cls).ravel()
    tested = [j for j in range(a.size) if cls[j] != UNTESTED]
    m = len(tested)
    out, R = np.where(cls == UNTESTED, NA, 0.0), np.zeros(a.shape, np.int64)
    c = 10.0 * np.log10(2.0) if two_sided else 0.0

    def B(j):
        return a[j] - 10.0 * np.log10(m / sum(1 for t in tested if a[t] >= a[j])) - c

    for i in tested:
        if a[i] > 0:
            R[i] = sum(1 for t in tested if a[t] >= a[i])
            A = max(0.0, max(B(j) for j in tested if 0 < a[j] <= a[i]))
            out[i] = (-A if cls[i] == MINUS else A) + 0.0
    return out, m, R


def compare(got_a, got_m, got_rank, A, m, R, tol=1e-5):
    """Assert an implementation's outputs against a model result (A, m, R): m and rank exact; the tested mask, NA and +0 exact, the sign
    exact (a value within tol of 0 may round to +0 on either side); |dA| <= tol; no -0 anywhere.  Returns the worst |dA|."""
    got_a = np.asarray(got_a, np.float32)
    assert got_a.shape == A.shape
    assert np.array_equal(np.asarray(got_m, np.int64), m), (got_m, m)
    if got_rank is not None:
        assert np.array_equal(np.asarray(got_rank, np.int64), R)
    assert np.array_equal(got_a == np.float32(NA), A == NA)
    assert not (np.signbit(got_a) & (got_a == 0)).any(), "-0 stored"
    assert (got_a[A == 0] == 0).all()
    big = np.abs(A) > tol
    assert np.array_equal(np.sign(got_a)[big], np.sign(A)[big])
    d = np.abs(got_a.astype(np.float64) - A)
    worst = float(d.max()) if d.size else 0.0
    assert worst <= tol, worst
    return worst


def check(got_a, got_m, got_rank, s, two_sided, tol=1e-5):
    """compare() against the model of the plane s."""
    return compare(got_a, got_m, got_rank, *adjust(s, two_sided), tol=tol)


# ---- the command line's files (AmpliSolveFalseDiscovery, csrc/host/run_fd.cpp) ------------------------------------------------------------

def format_files(names, n_normals, positions, ref_code, trecs, q, params):
    """FDR_Calls.txt, FDR_Samples.txt and FDR_Summary.txt as text.  names: the tumours'; positions [(chrom, coordinate)]; ref_code [P];
    trecs int32 [T][>= P][8]; q float32 [T][P][4][2], the plane of ampli_nb_score_records; params: C_value, coverage_cutoff,
    calling_cutoff, fdr, q_min.  A cell is listed iff (float32)A >= a_min = -10 log10(fdr)."""
    P, q_min, fdr = len(positions), float(params["q_min"]), float(params["fdr"])
    a_min = -10.0 * np.log10(fdr)
    q = np.asarray(q, np.float32)
    A, m, R = adjust(q, False)
    A32 = A.astype(np.float32)
    calls = "sample\tchrom\tposition\tsubstitution\tXfw\tXrs\tFW\tBW\tQ_fw\tQ_rs\tKey\tA\tq\tRank\tRawGate\n"
    samples = "sample\tTested\tRawGate\tAdjusted\tRawOnly\tMinKey\n"
    tot = [0, 0, 0, 0]
    for t, name in enumerate(names):
        raw_n = adj_n = only_n = 0
        min_key = None
        for p in range(P):
            r = np.asarray(trecs[t, p], np.int64)
            for y in range(4):
                if A[t, p, y] == NA:
                    continue
                raw = bool(q[t, p, y, 0] >= q_min and q[t, p, y, 1] >= q_min)
                found = bool(float(A32[t, p, y]) >= a_min)
                raw_n += raw
                only_n += raw and not found
                if not found:
                    continue
                adj_n += 1
                key = float(min(q[t, p, y, 0], q[t, p, y, 1]))
                min_key = key if min_key is None else min(min_key, key)
                a = float(A32[t, p, y])
                calls += (f"{name}\t{positions[p][0]}\t{positions[p][1]}\t{'ACGT'[ref_code[p]]}->{'ACGT'[y]}\t{r[y]}\t{r[4 + y]}\t{r[:4].sum()}\t{r[4:].sum()}\t"
                          f"{q[t, p, y, 0]:.6f}\t{q[t, p, y, 1]:.6f}\t{key:.6f}\t{a:.6f}\t{10.0 ** (-a / 10.0):.6g}\t{R[t, p, y]}\t{'PASS' if raw else 'FAIL'}\n")
        samples += f"{name}\t{m[t]}\t{raw_n}\t{adj_n}\t{only_n}\t{'NA' if min_key is None else f'{min_key:.6f}'}\n"
        tot = [tot[0] + int(m[t]), tot[1] + raw_n, tot[2] + adj_n, tot[3] + only_n]
    summary = (f"normals={n_normals}\ntumours={len(names)}\npositions={P}\nC_value={params['C_value']:g}\ncoverage_cutoff={params['coverage_cutoff']}\n"
               f"calling_cutoff={params['calling_cutoff']}\nfdr={fdr:g}\na_min={a_min:.6g}\nq_min={q_min:g}\ntested={tot[0]}\nraw_gate={tot[1]}\n"
               f"adjusted={tot[2]}\nraw_only={tot[3]}\n")
    return {"FDR_Calls.txt": calls, "FDR_Samples.txt": samples, "FDR_Summary.txt": summary}
