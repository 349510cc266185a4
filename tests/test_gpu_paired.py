"""Context.pair_score (paired_score_kernel) against the definition (tests/paired_model.py).  The evaluated mask, the sign, +0 and NA
are exact; S is held to 1e-5 (tests/test_paired_host.py derives it).  The cohorts come from tests/dispersion_cohorts.cohort: absent
records, positions listed twice (E > 0), an RD plane, a padded row stride -- none of which may change a score, since only the primary
record of (row, position) enters."""
import functools
import os

import numpy as np
import pytest

from tests.dispersion_cohorts import cohort
from tests.helpers import GOLDEN
from tests.paired_model import D_MAX, NA, score_model
from tests.test_gpu_overdispersion import _chunks
from tests.test_gpu_parity import _t

pytestmark = pytest.mark.gpu
S_TOL = 1e-5
CUTOFF = 30
ROWS_A, ROWS_B = 6, 5


def _pairs(kind, n_pairs, rng):
    """same: rows of one chunk, a self-pair among them from three pairs on; different: a row of A and a row of B; with more pairs than
    rows a row occurs in several pairs either way"""
    if kind == "same":
        out = [(int(a), int(b)) for a, b in zip(rng.integers(0, ROWS_A, n_pairs), rng.integers(0, ROWS_A, n_pairs))]
        out[0] = (1, 4)
        if n_pairs >= 3:
            out[2] = (3, 3)
        return out
    return [(i % ROWS_A, (2 * i + i // ROWS_B) % ROWS_B) for i in range(n_pairs)]


@functools.lru_cache(maxsize=None)
def _case(P, n_pairs, kind):
    rng = np.random.default_rng(11 * P + n_pairs)
    A = cohort(P, ROWS_A, 3 * P + n_pairs, extras=True, own_rd=True, u16=True)
    B = cohort(P, ROWS_B, 5 * P + n_pairs + 1, extras=True, own_rd=True, u16=True) if kind == "different" else A
    ref = rng.integers(0, 4, P).astype(np.uint8)
    ref[rng.random(P) < 0.08] = 255
    ref[rng.random(P) < 0.05] = 4
    pairs = _pairs(kind, n_pairs, rng)
    s, s64 = score_model(A[0], B[0], P, pairs, ref, CUTOFF)
    return A, B, ref, pairs, s, s64


def _records(ctx, c, P, layout, pad=0):
    recs, E, dup_off, ext_pos, rd = c
    return _chunks(ctx, recs, P, E, dup_off, ext_pos, None if layout == "u16" else rd, layout, (0, recs.shape[0]), pad=pad)[0]


def _same(got, want, want64):
    assert np.array_equal(got == NA, want == NA)                                   # the evaluated mask
    assert np.array_equal(np.sign(got), np.sign(want))                             # the side
    zero = want == 0
    assert (got[zero] == 0).all() and not np.signbit(got[zero]).any()             # +0, never -0
    ev = want != NA
    err = np.abs(got.astype(np.float64) - want64)[ev]
    assert (err <= S_TOL).all(), err.max()
    return float(err.max()) if ev.any() else 0.0


@pytest.mark.parametrize("layout", ["i32", "u24", "u16"])
@pytest.mark.parametrize("kind", ["same", "different"])
@pytest.mark.parametrize("P,n_pairs", [(1, 1), (63, 3), (64, 5), (65, 9), (130, 9), (1000, 3)])
def test_s_equals_the_model(ctx, layout, kind, P, n_pairs):
    A, B, ref, pairs, want, want64 = _case(P, n_pairs, kind)
    ra = _records(ctx, A, P, layout, pad=3 if n_pairs == 5 else 0)
    rb = _records(ctx, B, P, layout) if kind == "different" else ra
    d_pairs, d_ref = _t(np.array(pairs, np.int32)), _t(ref)
    got = ctx.pair_score(ra, rb, P, d_pairs, d_ref, CUTOFF).cpu().numpy()
    worst = _same(got, want, want64)
    again = ctx.pair_score(ra, rb, P, d_pairs, d_ref, CUTOFF).cpu().numpy()
    assert again.tobytes() == got.tobytes()                                        # the same inputs give the same bytes
    if P >= 63:
        ev = want != NA
        print(f"worst |S - model| {worst:.3g} over {int(ev.sum())} evaluated scores")
        assert (~ev).sum() > ev.sum() // 8 and (want[ev] == 0).any() and (want > 0).any() and (want < 0).any() and (np.abs(want) == 100).any()
        assert ((np.abs(want) > 0) & (np.abs(want) < 100)).sum() > 100
    if kind == "same" and n_pairs >= 3:  # the self-pair: exactly +0 in every evaluated cell and NA elsewhere
        self_pair = got[2]
        assert ((self_pair == 0) | (self_pair == NA)).all() and (self_pair == 0).sum() == (want[2] != NA).sum() and not np.signbit(self_pair[self_pair == 0]).any()


def test_a_row_in_several_pairs_and_rows_out_of_range(ctx):
    """row 2 of A against every row of B, twice over, and pairs that name a row outside either chunk -- all NA, no record loaded"""
    P = 65
    A, B, ref, _, _, _ = _case(P, 9, "different")
    pairs = [(2, b) for b in range(ROWS_B)] + [(ROWS_A, 0), (0, ROWS_B), (-1, 1), (1, -1), (2 ** 31 - 1, 0), (-2 ** 31, -2 ** 31)] + [(2, b) for b in range(ROWS_B)]
    want, want64 = score_model(A[0], B[0], P, pairs, ref, CUTOFF)
    ra, rb = _records(ctx, A, P, "u16"), _records(ctx, B, P, "u16")
    got = ctx.pair_score(ra, rb, P, _t(np.array(pairs, np.int32)), _t(ref), CUTOFF).cpu().numpy()
    _same(got, want, want64)
    assert (got[ROWS_B:ROWS_B + 6] == NA).all() and (want[ROWS_B:ROWS_B + 6] == NA).all()
    assert got[:ROWS_B].tobytes() == got[ROWS_B + 6:].tobytes() and (got[:ROWS_B] != NA).any()


def test_cutoff_sweep_per_strand_and_file(ctx):
    """any of the four strand depths at depth_cutoff - 1 makes the record NA, all four at the cut-off are scored"""
    P = 5
    recs = np.zeros((2, P, 8), np.int32)
    for p, (fa, ba, fb, bb) in enumerate(((99, 100, 100, 100), (100, 99, 100, 100), (100, 100, 99, 100), (100, 100, 100, 99), (100, 100, 100, 100))):
        recs[0, p] = [fa - 9, 9, 0, 0, ba - 7, 7, 0, 0]
        recs[1, p] = [fb - 1, 1, 0, 0, bb, 0, 0, 0]
    r = ctx.records(_t(recs), "i32", 2)
    pairs, ref = _t(np.array([[0, 1]], np.int32)), _t(np.zeros(P, np.uint8))
    s = ctx.pair_score(r, r, P, pairs, ref, 100).cpu().numpy()
    assert (s[0, :4] == NA).all() and (s[0, 4, 0] == NA).all() and (s[0, 4, 1] > 0).all() and (s[0, 4, 2:] == 0).all()
    s = ctx.pair_score(r, r, P, pairs, ref, 99).cpu().numpy()
    assert (s[0, :, 1] > 0).all() and (s[0, :, 0] == NA).all()


def test_grid_corners_in_records(ctx):
    """the recorded grid's corner tables (depths up to 2^31 - 1, the longest sums, the clamp on both signs) packed into int32 records
    and scored on the device: a on row 0, b on row 1, the same table on both strands"""
    g = np.load(os.path.join(GOLDEN, "paired", "hyper_grid.npz"))
    k_a, d_a, k_b, d_b, want = g["k_a"], g["d_a"], g["k_b"], g["d_b"], g["s"]
    big = np.nonzero((d_a >= 1000003) | (d_b >= 1000003))[0]
    rest = np.nonzero((np.abs(want) > 99) | ((d_a < 8) & (d_b < 8)))[0]
    pick = np.unique(np.concatenate([big[:400], big[-200::3], rest[::3]]))
    P = len(pick)
    assert P >= 500 and d_a[pick].max() == D_MAX and d_b[pick].max() == D_MAX and (want[pick] == 100).any() and (want[pick] == -100).any()
    recs = np.zeros((2, P, 8), np.int32)
    for row, (k, d) in enumerate(((k_a, d_a), (k_b, d_b))):
        recs[row, :, 0] = d[pick] - k[pick]
        recs[row, :, 1] = k[pick]
        recs[row, :, 4:] = recs[row, :, :4]
    r = ctx.records(_t(recs), "i32", 2)
    s = ctx.pair_score(r, r, P, _t(np.array([[0, 1], [1, 0]], np.int32)), _t(np.zeros(P, np.uint8)), 0).cpu().numpy()
    err = np.abs(s[0, :, 1, :].astype(np.float64) - want[pick][:, None])
    print("corners: worst |S - model|", err.max(), "over", P, "tables")
    assert (err <= S_TOL).all() and (s[:, :, 0] == NA).all() and (s[:, :, 2:] == 0).all()
    assert np.array_equal(np.sign(s[0, :, 1, 0]), np.sign(want[pick]).astype(np.float32))
    # S(b, a) = -S(a, b): the other file's tail is another sum, held to the same tolerance; +0 stays +0
    assert (np.abs(s[1, :, 1, :].astype(np.float64) + want[pick][:, None]) <= S_TOL).all() and not np.signbit(s[s == 0]).any()
