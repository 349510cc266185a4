"""Panels, variant lists and records for the monitoring tests -- TEST INFRASTRUCTURE shared by the host and the GPU tests.
Everything is computed once per shape and read-only."""
import functools

import numpy as np

from tests.concordance_cohorts import records
from tests.monitor_model import ABSENT, candidates, controls_model, sums_model

LENGTHS = (0, 1, 63, 64, 65, 130, 257, 300)  # the register form (up to 256 entries), its edge, and the rounds form
COV = 100


@functools.lru_cache(maxsize=None)
def panel(P, seed=5):
    """thr float32 [2, 4, P] and ref_code uint8 [P]: thresholds around 1e-3 with -1 on one strand only, -1 on both, 0 and a NaN planted;
    reference codes 0..3 with a few 4 ("N") and 255"""
    rng = np.random.default_rng(seed + P)
    thr = np.exp(rng.uniform(np.log(2e-4), np.log(5e-3), (2, 4, P))).astype(np.float32)
    kind = rng.integers(0, 12, (4, P))
    thr[0][kind == 0] = -1.0   # no estimate on the forward strand only
    thr[1][kind == 1] = -1.0   # ... on the backward strand only
    thr[:, kind == 2] = -1.0
    thr[0][kind == 3] = 0.0    # replaced by 0.0010008f
    thr[:, kind == 4] = 0.0
    thr[1][kind == 5] = np.nan
    ref = rng.integers(0, 4, P).astype(np.uint8)
    odd = rng.random(P) < 0.06
    ref[odd] = rng.choice(np.array([4, 255], np.uint8), int(odd.sum()))
    if P == 1:
        ref[0], thr[:, :, 0] = 2, np.float32(1e-3)
    thr.setflags(write=False)
    ref.setflags(write=False)
    return thr, ref


@functools.lru_cache(maxsize=None)
def lists(P, seed=7):
    """list_off, list_cell (uint32): LENGTHS drawn at random from the cells of [0, P) -- unsorted, overlapping, with repeats, y == ref
    among them --, then a list that names one cell twice, one of entries with p >= P only, one that mixes both, and the whole panel's
    cells in order"""
    rng = np.random.default_rng(seed + P)
    parts = [rng.integers(0, 4 * P, n) for n in LENGTHS]
    c = int(rng.integers(0, 4 * P))
    parts += [np.array([c, c]), 4 * (P + rng.integers(0, 1000, 5)) + 1, np.concatenate([rng.integers(0, 4 * P, 70), 4 * (P + rng.integers(0, 9, 3))]),
              np.arange(4 * P)]
    off = np.concatenate([[0], np.cumsum([len(x) for x in parts])]).astype(np.uint32)
    cell = np.concatenate(parts).astype(np.uint32)
    off.setflags(write=False)
    cell.setflags(write=False)
    return off, cell


@functools.lru_cache(maxsize=None)
def cohort(P, n, seed=11):
    """recs int32 [n, P, 8] with absent records and strands around the cut-off (the boundary grid of the concordance tests), and, at
    the first listed cells that can be evaluated, planted records: one strand one read below the cut-off, and the allele-fraction gate
    at equality and one read beyond (with max_vaf_pm = 250)"""
    recs = records(P, n, seed + 16 * P + n).copy()
    thr, ref = panel(P)
    off, cell = lists(P)
    good = [int(c) for c in cell[: int(off[len(LENGTHS)])] if ref[int(c) >> 2] <= 3 and (int(c) & 3) != ref[int(c) >> 2]]
    for k, (fw, bw, kf, kb) in enumerate([(COV - 1, COV, 0, 0), (COV, COV - 1, 1, 0), (COV, COV, 0, 0), (400, 400, 100, 100), (400, 400, 101, 100),
                                          (400, 400, 100, 101), (1000, 3000, 0, 1000), (1000, 3000, 1, 1000)]):
        if k >= len(good):
            break
        p, y = good[k] >> 2, good[k] & 3
        r = np.zeros(8, np.int32)
        o = (y + 1) & 3
        r[y], r[4 + y], r[o], r[4 + o] = kf, kb, fw - kf, bw - kb
        recs[k % n, p] = r
    recs.setflags(write=False)
    return recs


@functools.lru_cache(maxsize=None)
def expected(P, n, max_vaf_pm=1000):
    recs = cohort(P, n)
    thr, ref = panel(P)
    off, cell = lists(P)
    sums, lam = sums_model(recs, P, thr, ref, off, cell, COV, max_vaf_pm)
    sums.setflags(write=False)
    lam.setflags(write=False)
    return sums, lam


CONTROL_SEED = 0x5EED0BADC0FFEE11


@functools.lru_cache(maxsize=None)
def control_case(P, n, R, first_rep=0, empty_class=None, single=False):
    """pairs int32 [n_pairs, 2], cand_off, cand_pos and the model's sums for R replicates from first_rep.  The pairs name every kind of
    list, two rows with the same list, and a row and a list out of range.  empty_class: a reference base without candidates; single:
    one candidate per base (m = 1)"""
    recs = cohort(P, n)
    thr, ref = panel(P)
    off, cell = lists(P)
    L = len(off) - 1
    cand_off, cand_pos = candidates(ref)
    if single:
        keep = [cand_pos[int(cand_off[g]):int(cand_off[g + 1])][:1] for g in range(4)]
        cand_off, cand_pos = np.concatenate([[0], np.cumsum([len(x) for x in keep])]).astype(np.uint32), np.concatenate(keep).astype(np.uint32)
    if empty_class is not None:
        g = empty_class
        lo, hi = int(cand_off[g]), int(cand_off[g + 1])
        cand_pos = np.concatenate([cand_pos[:lo], cand_pos[hi:]])
        cand_off = cand_off.astype(np.int64)
        cand_off[g + 1:] -= hi - lo
        cand_off = cand_off.astype(np.uint32)
    pairs = [(0, 2), (n - 1, 2), (0, 5), (n - 1, 6), (0, 7), (0, 0), (0, 8), (n // 2, 10), (0, 9), (n, 2), (0, L), (-1, 3), (0, -1)]
    pairs = np.array(pairs, np.int32)
    sums, lam = controls_model(recs, P, thr, ref, off, cell, pairs, cand_off, cand_pos, R, first_rep, CONTROL_SEED, COV, 1000)
    for a in (pairs, cand_off, cand_pos, sums, lam):
        a.setflags(write=False)
    return pairs, cand_off, cand_pos, sums, lam


def big_records(P, n, seed=30):
    """int32 fields of 2^30 (a strand's depth beyond 2^31), 2^31 - 1, and absent records"""
    big, top = 1 << 30, (1 << 31) - 1
    menu = np.array([[big, big, big, 1 << 25, big, 0, big, 1 << 25], [top, top, top, top, top, top, top, top], [0, top, top >> 5, 0, 0, top, 0, 7],
                     [99, 0, 0, 0, top, top, 0, 0], [3, 0, 5, top, 0, 0, 0, 99], [ABSENT, top, 0, 0, top, 0, 0, 0]], np.int64).astype(np.int32)
    return menu[np.random.default_rng(seed).integers(0, len(menu), (n, P))]
