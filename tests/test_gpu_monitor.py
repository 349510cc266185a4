"""Context.monitor_sums / monitor_controls / monitor_score (ampli_monitor.hip) against the definition (tests/monitor_model.py): the
integers and Lambda exactly (np.array_equal on the int64 sums and on the doubles' bit patterns), Q bit for bit with the host library and
within 1e-5 of the 50-digit model.

Sums: lists of 0, 1, 63, 64, 65, 130, 257 and 300 entries (up to 256 a wave keeps its entries in registers, beyond it walks the list in
rounds of 64), a cell listed twice, entries with p >= P, the whole panel's cells; P = 1, 64, 65, 1000; n = 1, 3, 9 (one more than a
strip); every layout; a padded row stride; y == ref, reference codes above 3, a threshold of -1 on one strand only, of 0, a NaN; absent
records; one strand one read below the cut-off; the allele-fraction gate at equality and one read beyond; offsets beyond W; extras and
an RD plane without effect; int32 fields of 2^30.  Controls: R = 1, 7, 64, first_rep > 0 with two batches equal to one call, an empty
candidate class, m = 1, pair indices out of range, two samples with one control list.  Scores: the recorded grid, N_EVAL = 0, n_cells =
1, 63, 64, 65, 1000, and two runs with the same bytes."""
import numpy as np
import pytest

from amplisolve_amd.api import MON_NA, MON_STRIP
from tests import monitor_model as mm
from tests.monitor_cases import CONTROL_SEED, COV, big_records, cohort, control_case, expected, lists, panel
from tests.test_gpu_loo import _pack
from tests.test_gpu_parity import _t
from tests.test_monitor_host import GOLDEN, Q_BOUND, bits, host_score

pytestmark = pytest.mark.gpu
SHAPES = [(1, 1), (64, 3), (65, MON_STRIP + 1), (1000, 3), (1000, MON_STRIP + 1)]
assert MON_STRIP == 8


def _dev(P):
    thr, ref = panel(P)
    return _t(thr), _t(ref)


def _same(got, exp):
    sums, lam = got
    return np.array_equal(sums.cpu().numpy(), exp[0]) and np.array_equal(bits(lam.cpu().numpy()), bits(exp[1]))


@pytest.mark.parametrize("layout", ["i32", "u24", "u16"])
@pytest.mark.parametrize("P,n", SHAPES)
def test_sums_equal_the_model(ctx, layout, P, n):
    off, cell = lists(P)
    thr, ref = _dev(P)
    exp = expected(P, n)
    if P >= 64:
        assert (exp[0][:, 2:8, mm.N_EVAL] > 0).any(axis=0).all() and (exp[0][:, 9] == 0).all()
    sums, lam = ctx.monitor_sums(ctx.records(_pack(ctx, cohort(P, n), layout), layout, n), P, thr, ref, off, cell, cov=COV)
    assert sums.shape == (n, len(off) - 1, 6) and lam.shape == (n, len(off) - 1, 2) and _same((sums, lam), exp)
    q = ctx.monitor_score(sums, lam).cpu().numpy()
    assert q.shape == (n, len(off) - 1, 2) and np.array_equal(q.reshape(-1, 2).view(np.int32), host_score(exp[0], exp[1]).view(np.int32))
    assert (q[exp[0][:, :, mm.N_EVAL] == 0] == MON_NA).all()


@pytest.mark.parametrize("layout", ["i32", "u16"])
def test_the_allele_fraction_gate_at_equality_and_beyond(ctx, layout):
    P, n = 65, 9
    off, cell = lists(P)
    thr, ref = _dev(P)
    exp = expected(P, n, 250)
    assert (exp[0][:, :, mm.N_EVAL] < expected(P, n)[0][:, :, mm.N_EVAL]).any()
    assert _same(ctx.monitor_sums(ctx.records(_pack(ctx, cohort(P, n), layout), layout, n), P, thr, ref, off, cell, cov=COV, max_vaf_pm=250), exp)


@pytest.mark.parametrize("cov", [0, COV - 1, COV + 1, 30000])
def test_the_cut_off(ctx, cov):
    P, n = 65, 3
    off, cell = lists(P)
    thr, ref = panel(P)
    exp = mm.sums_model(cohort(P, n), P, thr, ref, off, cell, cov, 1000)
    assert _same(ctx.monitor_sums(ctx.records(_pack(ctx, cohort(P, n), "u24"), "u24", n), P, _t(thr), _t(ref), off, cell, cov=cov), exp)


@pytest.mark.parametrize("layout", ["i32", "u24", "u16"])
def test_a_padded_row_stride(ctx, layout):
    P, n, pad = 65, 9, 7
    recs = cohort(P + pad, n)  # the pad holds records too: they must not be read in place of the next row's
    off, cell = lists(P)
    thr, ref = panel(P)
    exp = mm.sums_model(recs[:, :P], P, thr, ref, off, cell, COV, 1000)
    assert _same(ctx.monitor_sums(ctx.records(_pack(ctx, recs, layout), layout, n, row_stride=P + pad), P, _t(thr), _t(ref), off, cell, cov=COV), exp)


@pytest.mark.parametrize("layout", ["i32", "u24"])
def test_extras_and_an_rd_plane_do_not_matter(ctx, layout):
    P, n, E = 65, 3, 9
    rng = np.random.default_rng(4)
    recs = np.concatenate([cohort(P, n), cohort(E, n)], axis=1)
    dup_off = np.concatenate([[0], np.cumsum(np.isin(np.arange(P), rng.choice(P, E, replace=False)))]).astype(np.uint32)
    ext_pos = np.repeat(np.arange(P), np.diff(dup_off.astype(np.int64))).astype(np.uint32)
    rd = np.where(rng.random((n, P + E)) < 0.3, 12345, mm.ABSENT).astype(np.int32)
    full = ctx.records(_pack(ctx, recs, layout), layout, n, E=E, dup_off=_t(dup_off), ext_pos=_t(ext_pos), rd=_t(rd[:, :P]), rd_ext=_t(rd[:, P:]))
    off, cell = lists(P)
    thr, ref = _dev(P)
    assert _same(ctx.monitor_sums(full, P, thr, ref, off, cell, cov=COV), expected(P, n))


def test_i32_fields_of_two_to_the_thirty(ctx):
    P, n = 65, 9
    recs = big_records(P, n)
    off, cell = lists(P)
    thr, ref = panel(P)
    exp = mm.sums_model(recs, P, thr, ref, off, cell, COV, 1000)
    assert (exp[0][:, :, mm.D_FW] > 1 << 36).any() and (recs == 1 << 30).any()
    assert _same(ctx.monitor_sums(ctx.records(_t(recs), "i32", n), P, _t(thr), _t(ref), off, cell, cov=COV), exp)


def test_offsets_beyond_W(ctx):
    """device lists are taken as they are: a list that runs over W is cut there, the ones behind it are empty"""
    P, n = 65, 3
    off, cell = lists(P)
    thr, ref = panel(P)
    W = int(off[6]) + 10
    exp = mm.sums_model(cohort(P, n), P, thr, ref, off, cell[:W], COV, 1000)
    assert (exp[0][:, 7:] == 0).all() and (exp[0][:, 6, 0] > 0).any()
    d_off, d_cell = _t(off.astype(np.int32)), _t(cell[:W].astype(np.int32))
    assert _same(ctx.monitor_sums(ctx.records(_t(cohort(P, n)), "i32", n), P, _t(thr), _t(ref), d_off, d_cell, cov=COV), exp)


@pytest.mark.parametrize("layout", ["i32", "u16"])
def test_chunks_into_the_rows_of_one_matrix_and_two_runs(ctx, layout):
    import torch

    P, n, cuts = 1000, 9, (0, 1, 8, 9)
    off, cell = lists(P)
    thr, ref = _dev(P)
    exp = expected(P, n)
    L = len(off) - 1
    sums = torch.full((n, L, 6), -1, dtype=torch.int64, device=ctx.device)
    lam = torch.full((n, L, 2), float("nan"), dtype=torch.float64, device=ctx.device)
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        ctx.monitor_sums(ctx.records(_pack(ctx, cohort(P, n)[lo:hi], layout), layout, hi - lo), P, thr, ref, off, cell, cov=COV, sums=sums[lo:hi], lam=lam[lo:hi])
    assert _same((sums, lam), exp)
    rec = ctx.records(_pack(ctx, cohort(P, n), layout), layout, n)
    one, two = ctx.monitor_sums(rec, P, thr, ref, off, cell, cov=COV), ctx.monitor_sums(rec, P, thr, ref, off, cell, cov=COV)
    assert one[0].cpu().numpy().tobytes() == two[0].cpu().numpy().tobytes() and one[1].cpu().numpy().tobytes() == two[1].cpu().numpy().tobytes()


# ---- controls ----

def _controls(ctx, P, n, layout, pairs, cand_off, cand_pos, R, first_rep, recs=None):
    off, cell = lists(P)
    thr, ref = _dev(P)
    rec = ctx.records(_pack(ctx, cohort(P, n) if recs is None else recs, layout), layout, n)
    return ctx.monitor_controls(rec, P, thr, ref, off, cell, _t(pairs), _t(cand_off.astype(np.int32)), _t(cand_pos.astype(np.int32)), R, first_rep=first_rep,
                                seed=CONTROL_SEED, cov=COV)


@pytest.mark.parametrize("layout", ["i32", "u24", "u16"])
@pytest.mark.parametrize("R,first_rep", [(1, 0), (7, 0), (3, 5)])
def test_controls_equal_the_model(ctx, layout, R, first_rep):
    P, n = 65, 3
    pairs, cand_off, cand_pos, exp_s, exp_l = control_case(P, n, R=R, first_rep=first_rep)
    got = _controls(ctx, P, n, layout, pairs, cand_off, cand_pos, R, first_rep)
    assert _same(got, (exp_s, exp_l)) and (exp_s[9:] == 0).all() and (exp_s[:5, :, mm.N_EVAL] > 0).any()
    q = ctx.monitor_score(*got).cpu().numpy()
    assert np.array_equal(q.reshape(-1, 2).view(np.int32), host_score(exp_s, exp_l).view(np.int32)) and (q[9:] == MON_NA).all()


def test_sixty_four_replicates_and_two_batches_equal_one_call(ctx):
    import torch

    P, n, R, first = 65, 3, 64, 3
    pairs, cand_off, cand_pos, exp_s, exp_l = control_case(P, n, R=R, first_rep=first)
    one = _controls(ctx, P, n, "u16", pairs, cand_off, cand_pos, R, first)
    assert _same(one, (exp_s, exp_l))
    a = _controls(ctx, P, n, "u16", pairs, cand_off, cand_pos, 7, first)
    b = _controls(ctx, P, n, "u16", pairs, cand_off, cand_pos, R - 7, first + 7)
    assert torch.equal(torch.cat([a[0], b[0]], 1), one[0]) and torch.equal(torch.cat([a[1], b[1]], 1).view(torch.int64), one[1].view(torch.int64))


@pytest.mark.parametrize("kw", [dict(empty_class=1), dict(single=True)])
def test_an_empty_candidate_class_and_a_single_candidate(ctx, kw):
    P, n, R = 65, 3, 2
    pairs, cand_off, cand_pos, exp_s, exp_l = control_case(P, n, R=R, **kw)
    assert _same(_controls(ctx, P, n, "i32", pairs, cand_off, cand_pos, R, 0), (exp_s, exp_l))


def test_two_samples_share_their_control_lists(ctx):
    """a control list depends on (seed, list, replicate) only: two rows with the same records get the same cells"""
    P, n, R = 65, 3, 7
    recs = cohort(P, n).copy()
    recs[n - 1] = recs[0]
    pairs, cand_off, cand_pos, _, _ = control_case(P, n, R=R)
    assert tuple(pairs[0]) == (0, 2) and tuple(pairs[1]) == (n - 1, 2)
    sums, lam = _controls(ctx, P, n, "i32", pairs, cand_off, cand_pos, R, 0, recs=recs)
    sums, lam = sums.cpu().numpy(), lam.cpu().numpy()
    assert np.array_equal(sums[0], sums[1]) and np.array_equal(bits(lam[0]), bits(lam[1])) and (sums[0][:, mm.N_EVAL] > 0).any()
    assert len({sums[0][r].tobytes() for r in range(R)}) > 1  # the replicates differ


# ---- scores ----

@pytest.mark.parametrize("n_cells", [1, 63, 64, 65, 1000])
def test_scores_on_the_recorded_grid(ctx, n_cells):
    g = np.load(GOLDEN)
    n_grid = int(g["n_grid"])
    pick = np.linspace(0, n_grid - 1, n_cells).astype(np.int64) if n_cells <= n_grid else np.arange(n_cells)  # beyond the grid: the random vectors too
    K, lam, q = g["K"][pick], g["lam"][pick], g["q"][pick]
    sums = np.zeros((n_cells, 6), np.int64)
    sums[:, mm.N_EVAL], sums[:, mm.K_FW], sums[:, mm.K_BW] = 1, K, K[::-1]
    sums[::5, mm.N_EVAL] = 0
    lam2 = np.ascontiguousarray(np.stack([lam, lam[::-1]], 1))
    one = ctx.monitor_score(_t(sums), _t(lam2)).cpu().numpy()
    two = ctx.monitor_score(_t(sums), _t(lam2)).cpu().numpy()
    assert one.tobytes() == two.tobytes() and np.array_equal(one.view(np.int32), host_score(sums, lam2).view(np.int32))
    assert (one[::5] == MON_NA).all()
    live = sums[:, mm.N_EVAL] > 0
    assert np.abs(one[live, 0].astype(np.float64) - q[live]).max(initial=0.0) <= Q_BOUND
    if n_cells == 1000:
        assert lam.max() == 1e6 and (q[live] == 100).any() and ((q[live] > 0) & (q[live] < 100)).sum() > 300
