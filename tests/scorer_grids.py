"""The points at which the three Poisson scorers (csrc/ampli_math.h: ampli_poisson_score, ampli_poisson_score_dense, ampli_drain_p)
are compared with the oracle's literal scorer -- on the host (tests/test_math_host.py, every point) and on the device
(tests/test_gpu_scorer_domain.py, a fixed subsample of the two grids and every edge point).  Every function returns
(k int32, rd int32, err float32).  A count beyond the int32 range is clamped to INT32_MAX, which is a point like any other."""
import os

import numpy as np

INT32_MAX = (1 << 31) - 1
INT32_MIN = -(1 << 31)
MAGIC_ERR = float(np.float32(0.0010008))  # what an error of 0 stands for (VC:3852-3856)
HORNER_BOUND = 838860.8                   # ampli_poisson_p_dense: the closed form of the fraction's side ends here
LGTAB = 65537                             # AMPLI_LGTAB: kf_lgamma at 0 .. 65536 comes from the table
COUNT_LIMIT = 1 << 24                     # AMPLI_COUNT_LIMIT
GPU_POINTS = 150_000                      # of each grid on the device: the oracle's call is the slow part of those tests


def _pack(ks, rds, es):
    return np.concatenate(ks).astype(np.int32), np.concatenate(rds).astype(np.int32), np.concatenate(es).astype(np.float32)


def drain_grid():
    """Queued items of the drain (k > m = rd * err > 0), from just above the mean -- slow convergence, the region where the
    99-term cap cuts the series -- to far above it (Q = 100), at depths from 25 to 10^9."""
    rng = np.random.default_rng(8)
    ks, rds, es = [], [], []
    for err in (0.0001, 0.0005, 0.002, 0.002189, 0.0035, 0.01, 0.02, 0.05, 0.25):
        for scale in (50, 300, 1000, 2500, 25000, 400000, 3_000_000, 16_000_000, 500_000_000):
            rd = rng.integers(max(1, scale // 2), scale * 2, 600)
            m = rd * float(np.float32(err))
            # k from just above m (slow convergence, cap region) to far above it (Q = 100)
            for f in (1.0, 1.01, 1.1, 1.5, 3.0, 10.0):
                k = np.maximum(np.floor(m * f).astype(np.int64) + rng.integers(1, 4, rd.size), 1)
                ks.append(np.minimum(k, INT32_MAX)); rds.append(rd); es.append(np.full(rd.size, err))
    k, rd, e = _pack(ks, rds, es)
    keep = k.astype(np.float64) > rd.astype(np.float64) * e.astype(np.float64)
    return k[keep], rd[keep], e[keep]


def dense_grid():
    """What the all-scores mode scores: the reference's own golden grid, counts around the mean at every depth (both branches of
    kf_gammaq, the identity step j = s of the continued fraction, the 99-step caps of both loops, k and m far beyond 100), the
    special error codes, and small counts against small means (what a 2000x panel holds)."""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vc_scorer_reference.npz"))
    rng = np.random.default_rng(21)
    ks, rds, es = [g["k"].astype(np.int64)], [g["rd"].astype(np.int64)], [g["err"].astype(np.float64)]
    for err in (0.0, -1.0, 0.0001, 0.0005, 0.002, 0.002189, 0.0035, 0.01, 0.02, 0.05, 0.25, 0.9):
        for scale in (1, 5, 50, 300, 1000, 2500, 25000, 400000, 3_000_000, 16_000_000, 500_000_000):
            rd = rng.integers(max(1, scale // 2), scale * 2 + 1, 400)
            m = rd * float(np.float32(err if err > 0 else 0.0010008))
            for f in (0.0, 0.3, 0.8, 0.97, 1.0, 1.03, 1.3, 3.0, 10.0):
                k = np.maximum(np.floor(m * f).astype(np.int64) + rng.integers(-2, 3, rd.size), 0)
                ks.append(np.minimum(k, INT32_MAX)); rds.append(rd); es.append(np.full(rd.size, err))
    # small counts x small means: what a 2000x panel holds
    kk, mm = np.meshgrid(np.arange(0, 40), np.arange(1, 120), indexing="ij")
    ks.append(kk.ravel()); rds.append(mm.ravel() * 50); es.append(np.full(kk.size, 0.002))
    return _pack(ks, rds, es)


def subsample(k, rd, e, n=GPU_POINTS, seed=77):
    """At most n points of a grid, the same ones on every run"""
    if k.size <= n:
        return k, rd, e
    idx = np.sort(np.random.default_rng(seed).choice(k.size, n, replace=False))
    return k[idx], rd[idx], e[idx]


def table_end_points():
    """Counts on both sides of the lgamma table's last entry (index 65536) at a threshold of 0.25, on both sides of the mean, so
    that the series reads kf_lgamma(k + 1) and the continued fraction kf_lgamma(k) across the table's end.  Above the mean
    (depths around 260 000: m = k - 2.1 sqrt(k)) Q lies strictly between 5 and 100 (asserted from the oracle where these points are
    used); below the mean p is close to 1 in exact arithmetic, and what the reference's 99-step cap makes of it there is part of
    the reference's result."""
    ks, rds, es = [], [], []
    for k in (65534, 65535, 65536, 65537, 65538):
        for dm in (-536, -300, -100, 100, 536):  # mean - count
            ks.append([k]); rds.append([4 * (k + dm)]); es.append([0.25])
    k, rd, e = _pack(ks, rds, es)
    above = k.astype(np.float64) > rd.astype(np.float64) * e.astype(np.float64)
    return k, rd, e, above


BIG = (COUNT_LIMIT - 1, COUNT_LIMIT, COUNT_LIMIT + 1, 1 << 30, INT32_MAX - 1, INT32_MAX)
BIG_ERRS = (1e-5, 0.002, 0.0, 0.25, 0.9, -1.0)


def edge_points():
    """The explicit edges, beyond table_end_points():
      * counts and depths at and beyond AMPLI_COUNT_LIMIT = 2^24 up to INT32_MAX, against six errors (0 = the magic 0.0010008f,
        -1 = no estimate);
      * means on both sides of the bound of the closed form (z < 838860.8) with k = 1 .. 5 (AMPLI_HORNER_K = 4);
      * k = 0; rd = 0 (z = 0: the series gives p = 0, Q = 100);
      * negative counts (the literal path of the all-scores form);
      * negative depths and a negative error that is not -1 (z <= 0: NaN in the reference)."""
    ks, rds, es = [], [], []
    for k in BIG:
        for rd in BIG:
            for err in BIG_ERRS:
                ks.append([k]); rds.append([rd]); es.append([err])
    for rd in BIG:  # and counts next to the mean of those depths, where p is neither 0 nor 1
        for err in BIG_ERRS[:-1]:
            m = rd * float(np.float32(err if err > 0 else 0.0010008))
            for dk in (-1, 0, 1, 3, int(3 * np.sqrt(m))):
                ks.append([min(int(np.floor(m)) + dk, INT32_MAX)]); rds.append([rd]); es.append([err])
    for err, rd_lo in ((0.25, 3355443), (0.5, 1677721), (0.05, 16777215)):  # rd_lo * err < 838860.8 <= (rd_lo + 1) * err
        assert rd_lo * float(np.float32(err)) < HORNER_BOUND <= (rd_lo + 1) * float(np.float32(err))
        for rd in (rd_lo - 1, rd_lo, rd_lo + 1, rd_lo + 2):
            for k in (1, 2, 3, 4, 5):
                ks.append([k]); rds.append([rd]); es.append([err])
    for rd in (0, 1, 500, 100_000, COUNT_LIMIT, INT32_MAX):
        for err in (0.002, 0.0, 0.25, -1.0):
            ks.append([0]); rds.append([rd]); es.append([err])
    for k in (0, 1, 2, 77, 65536, 65537, COUNT_LIMIT, INT32_MAX):
        for err in (0.002, 0.0, 0.25, -1.0):
            ks.append([k]); rds.append([0]); es.append([err])
    for k in (-1, -2, -77, -65537, -COUNT_LIMIT, INT32_MIN + 1, INT32_MIN):
        for rd in (0, 1, 500, 100_000, INT32_MAX):
            for err in (0.002, 0.0, 0.25, -1.0):
                ks.append([k]); rds.append([rd]); es.append([err])
    for k in (0, 1, 5, 300, 65537, INT32_MAX):
        for rd, err in ((-1, 0.002), (-500, 0.25), (INT32_MIN, 0.002), (-COUNT_LIMIT, 0.0), (500, -0.002), (100_000, -0.25), (INT32_MAX, -1e-5),
                        (-500, -0.002), (-500, -1.0)):
            ks.append([k]); rds.append([rd]); es.append([err])
    return _pack(ks, rds, es)


def in_drain_domain(k, rd, e):
    """0 < m < k with the effective error: what the drain's scorer is asked (drain_body, csrc/ampli_device.h)"""
    ee = np.where(e == 0, np.float32(0.0010008), e).astype(np.float32)
    m = rd.astype(np.float64) * ee.astype(np.float64)
    return (e != -1) & (m > 0) & (k.astype(np.float64) > m)


# ---- the comparison with the oracle's literal scorer, the same on the host and on the device -------------------------------------------
Q_TOL = 1e-6      # the project's contract on p, absolute and relative (tests/test_gpu_parity.py)
GATE_EPS = 1e-6   # AMPLI_CALL_GATE_EPS: a Q this close to a gate is re-decided by the host, by contract
MAX_IN_BAND = 1e-3  # of a set of points may lie that close to a gate


def gate_bands(qo, po):
    """Where the oracle's Q is within GATE_EPS of the gates 5, 20 and 100 (bool [3][n]).  Q = 100 is a clamp (p < 1e-10): the
    distance to that gate is taken on the unclamped -10 log10 p, so that only a p next to 1e-10 counts, not every clamped point."""
    with np.errstate(divide="ignore", invalid="ignore"):
        qu = np.where(po > 0, -10.0 * np.log10(np.where(po > 0, po, 1.0)), np.inf)  # p <= 0: as far beyond the clamp as can be
    fin = ~np.isnan(qo) & (qo != -888)
    return np.stack([fin & (np.abs(qo - 5.0) <= GATE_EPS), fin & (np.abs(qo - 20.0) <= GATE_EPS), fin & (np.abs(qu - 100.0) <= GATE_EPS)])


def compare_with_oracle(name, k, rd, e, qo, po, q, p=None, report=None):
    """One scorer's q (and p, where it returns one) at the points (k, rd, e) against the oracle's (qo, po):
      * the NaN pattern and the codes -888 and 0 are the oracle's; so is the clamp Q = 100 outside the band around that gate;
      * p within Q_TOL, absolute, and relative where p > 1e-10 (below it Q is clamped); Q within 1e-5 wherever neither is clamped;
      * the Q >= 5 / >= 20 / = 100 decisions are the oracle's wherever its Q is farther than GATE_EPS from the gate;
      * at most MAX_IN_BAND of the points lie in such a band (a property of the points: it depends on the oracle alone).
    A failure names k, rd and err.  Returns {depth decade: worst relative error of p} (p from Q where the scorer returns no p);
    report (a list) collects one line per decade."""
    def where(bad):
        i = int(np.flatnonzero(bad)[0])
        return f"{name}: k={int(k[i])} rd={int(rd[i])} err={float(e[i])!r}: q={q[i]!r} oracle {qo[i]!r}" + (
            f", p={p[i]!r} oracle {po[i]!r}" if p is not None else f", oracle p {po[i]!r}") + f" ({int(bad.sum())} such points)"

    bands = gate_bands(qo, po)
    share = float(bands.any(0).mean())
    assert share <= MAX_IN_BAND, f"{name}: {share:.2e} of the points lie within {GATE_EPS} of a gate"
    nan = np.isnan(qo)
    bad = np.isnan(q) != nan
    assert not bad.any(), where(bad)
    for code in (-888.0, 0.0):
        bad = (q == code) != (qo == code)
        assert not bad.any(), where(bad)
    for g, thr in enumerate((5.0, 20.0, 100.0)):
        bad = ~nan & ~bands[g] & ((q >= thr) != (qo >= thr))
        assert not bad.any(), where(bad)
    plain = ~nan & (qo != -888) & (qo != 0) & (qo != 100) & (q != 100)
    bad = plain & ~(np.abs(q - qo) <= 1e-5)
    assert not bad.any(), where(bad)
    if p is not None:
        bad = np.isnan(p) != np.isnan(po)
        assert not bad.any(), where(bad)
        ok = ~np.isnan(po)
        bad = ok & ~(np.abs(p - po) <= Q_TOL)
        assert not bad.any(), where(bad)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        pp = p if p is not None else np.where(plain, 10.0 ** (-q / 10), np.nan)
        big = ~np.isnan(po) & ~np.isnan(pp) & (np.abs(po) > 1e-10) & (e != -1)
        rel = np.where(big, np.abs(pp - po) / np.where(big, np.abs(po), 1.0), 0.0)
    worst = {}
    dec = np.floor(np.log10(np.maximum(np.abs(rd.astype(np.float64)), 1.0))).astype(np.int64)
    for d in np.unique(dec[big]):
        worst[int(d)] = float(rel[big & (dec == d)].max())
    for d, w in sorted(worst.items()):
        line = f"{name}: depth 1e{d}..: worst relative error of p {w:.3e} over {int((big & (dec == d)).sum())} points"
        print(line)
        if report is not None:
            report.append(line)
    if p is not None:  # after the report, so that a miss still shows the figures
        bad = big & ~(rel <= Q_TOL)
        assert not bad.any(), where(bad)
    return worst
