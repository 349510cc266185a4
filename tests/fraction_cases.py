"""Panel, weighted variant lists and records for the tumour-fraction tests -- TEST INFRASTRUCTURE shared by the host and the
GPU tests.  Everything is computed once per shape and read-only."""
import functools

import numpy as np

from tests.concordance_cohorts import records
from tests.fraction_model import Z2_95, fraction_model
from tests.monitor_cases import panel as monitor_panel

P = 300
ROWS = (1, 7, 8, 9, 17)                      # a strip is 8 rows: below it, at it, beyond it, and a third strip
LENGTHS = (0, 1, 63, 64, 65, 256, 257, 600)  # the register form (up to 256 entries), its edge, and the gathered form
COV = 100
REAL = 150       # positions [0, REAL): plasma-like records (depth 2500-3500 a strand, alternative reads at e + f a)
QUIET = (REAL, REAL + 3)         # no alternative read, thresholds 1e-4: F_HAT = 0 and F_HI > 0
FULL = (REAL + 3, REAL + 6)      # every read is the listed base: with weight 0.1 and the cap off U(1) >= 0, F_HAT = F_HI = 1
SILENT = (REAL + 6, REAL + 16)   # no alternative read under thresholds 1e-3: -T(0) >= z2, F_HI = 0
ROW_F = (0.0, 0.001, 0.01, 0.0003, 0.05, 0.0, 0.2, 0.003)  # the planted fraction of row s is ROW_F[s % 8]


@functools.lru_cache(maxsize=None)
def panel():
    """thr float32 [2, 4, P] and ref_code uint8 [P]: the monitoring tests' panel (thresholds around 1e-3 with -1 on one strand, on both, 0
    and a NaN planted; reference codes 0..3 with a few 4 and 255), with clean positions for the three planted lists"""
    thr, ref = (x.copy() for x in monitor_panel(P))
    for (lo, hi), e in ((QUIET, 1e-4), (FULL, 1e-3), (SILENT, 1e-3)):
        thr[:, :, lo:hi] = np.float32(e)
        ref[lo:hi] = np.arange(lo, hi) % 4
    thr.setflags(write=False)
    ref.setflags(write=False)
    return thr, ref


def _alt(p):
    """the listed base of the planted positions: the one after the reference base"""
    return (int(panel()[1][p]) + 1) & 3


@functools.lru_cache(maxsize=None)
def lists(seed=26):
    """list_off, list_cell (uint32) and list_w (float32): LENGTHS drawn at random from the cells of [0, P) -- unsorted, overlapping, with
    repeats, y == ref among them --, a list that names one cell twice, one of entries with p >= P only, one of plasma-like cells only,
    one whose weights are NaN, an infinity, 0, -0, negative and above 1 around two good ones, the three planted lists (QUIET, FULL,
    SILENT), and the whole panel's cells in order.  Weights are uniform in (0.05, 1], a few exactly 1."""
    rng = np.random.default_rng(seed)
    thr, ref = panel()
    real = np.array([4 * p + y for p in range(REAL) for y in range(4) if ref[p] <= 3 and y != ref[p]])
    parts = [rng.integers(0, 4 * P, n) for n in LENGTHS]
    c = int(real[5])
    bad = rng.choice(real[[bool(thr[0, c & 3, c >> 2] >= 0 and thr[1, c & 3, c >> 2] >= 0) for c in real]], 8, replace=False)  # thresholds that count
    parts += [np.array([c, c]), 4 * (P + rng.integers(0, 1000, 5)) + 1, rng.choice(real, 40, replace=False), bad,
              np.array([4 * p + _alt(p) for p in range(*QUIET)]), np.array([4 * p + _alt(p) for p in range(*FULL)]),
              np.array([4 * p + _alt(p) for p in range(*SILENT)]), np.arange(4 * P)]
    off = np.concatenate([[0], np.cumsum([len(x) for x in parts])]).astype(np.uint32)
    cell = np.concatenate(parts).astype(np.uint32)
    w = (1.0 - rng.uniform(0.0, 0.95, len(cell))).astype(np.float32)
    w[rng.random(len(cell)) < 0.02] = 1.0
    L0 = len(LENGTHS)
    w[int(off[L0 + 3]):int(off[L0 + 4])] = np.array([np.nan, 0.4, np.inf, 0.0, -0.0, -0.3, 1.5, 0.25], np.float32)
    w[int(off[L0 + 5]):int(off[L0 + 6])] = np.float32(0.1)
    for a in (off, cell, w):
        a.setflags(write=False)
    return off, cell, w


LIST_TWICE, LIST_BEYOND, LIST_REAL, LIST_BAD_W, LIST_QUIET, LIST_FULL, LIST_SILENT, LIST_ALL = range(len(LENGTHS), len(LENGTHS) + 8)


@functools.lru_cache(maxsize=None)
def cohort(n, seed=11):
    """recs int32 [n, P, 8]: positions [0, REAL) plasma-like at the row's planted fraction, with absent records and strands below the
    cut-off among them; the planted positions; the rest random records with the boundary grid of the concordance tests (absent records,
    strands around the cut-off)"""
    rng = np.random.default_rng(seed + n)
    recs = records(P, n, seed + 16 * P + n).copy()
    thr, ref = panel()
    for s in range(n):
        f = ROW_F[s % len(ROW_F)]
        for p in range(REAL):
            r = np.zeros(8, np.int64)
            g = int(ref[p]) & 3
            for st in range(2):
                d = int(rng.integers(2500, 3501))
                alt = rng.binomial(d, 0.0005 + f * 0.4, 3) if f < 0.1 else rng.binomial(d, [0.0005 + f * 0.4, 0.0005, 0.0005])
                r[4 * st + (g + 1 + np.arange(3)) % 4] = alt
                r[4 * st + g] = max(d - int(alt.sum()), 0)
            recs[s, p] = r
        kind = rng.random(REAL)
        recs[s, :REAL][kind < 0.03] = np.array([np.iinfo(np.int32).min, 0, 0, 0, 0, 0, 0, 0], np.int32)
        low = np.nonzero((kind >= 0.03) & (kind < 0.06))[0]
        recs[s, low] = np.array([COV - 1, 0, 0, 0, 1, 2, 3, 4000], np.int32)[None, :]  # one strand one read below the cut-off
        for lo, hi in (QUIET, SILENT):
            for p in range(lo, hi):
                r = np.zeros(8, np.int32)
                r[int(ref[p])], r[4 + int(ref[p])] = 3000 + s, 2900 + p
                recs[s, p] = r
        for p in range(*FULL):
            r = np.zeros(8, np.int32)
            r[_alt(p)], r[4 + _alt(p)] = 500 + s, 700 + p
            recs[s, p] = r
    recs.setflags(write=False)
    return recs


@functools.lru_cache(maxsize=None)
def expected(n, max_vaf_pm=1000, cov=COV, z2=Z2_95):
    thr, ref = panel()
    off, cell, w = lists()
    est, count = fraction_model(cohort(n), P, thr, ref, off, cell, w, cov, max_vaf_pm, z2)
    est.setflags(write=False)
    count.setflags(write=False)
    return est, count
