"""Context.tumour_fraction (ampli_fraction.hip) against the definition (tests/fraction_model.py): the four doubles bit for bit
(np.array_equal on their integer views) and the counts exactly, in all three record layouts.

P = 300; rows 1, 7, 8, 9 and 17 (a strip is 8 rows); lists of 0, 1, 63, 64, 65, 256, 257 and 600 entries (up to 256 a wave keeps its
entries in registers, beyond it gathers the list again for every evaluation) and the whole panel's 1200 cells; a cell listed twice;
entries with p >= P; weights NaN, infinite, 0, -0, negative and above 1; thresholds of -1, 0 and a NaN; y == ref and reference codes
above 3; rows below the coverage cut-off and absent records; the max_vaf_pm cap on and off; a list without an alternative read (F_HAT =
0, F_HI > 0); a list whose U(1) >= 0 (weight 0.1, every read the listed base, the cap off: F_HAT = F_HI = 1); a list with -T(0) >= z2
(F_HI = 0); a padded row stride; offsets beyond W; chunks into the rows of one matrix; int32 fields of 2^30 and 2^31 - 1.  The shared
cases are checked to take these branches in tests/test_fraction_host.py, which also holds the host library to the same bits."""
import numpy as np
import pytest

from tests import fraction_model as fm
from tests.fraction_cases import COV, LIST_FULL, LIST_QUIET, LIST_SILENT, P, ROWS, cohort, expected, lists, panel
from tests.monitor_cases import big_records
from tests.test_fraction_host import bits, same
from tests.test_gpu_loo import _pack
from tests.test_gpu_parity import _t

pytestmark = pytest.mark.gpu


def _dev():
    thr, ref = panel()
    off, cell, w = lists()
    return _t(thr), _t(ref), off, cell, w


def _got(pair):
    return pair[0].cpu().numpy(), pair[1].cpu().numpy()


@pytest.mark.parametrize("layout", ["i32", "u24", "u16"])
@pytest.mark.parametrize("n", ROWS)
def test_the_device_equals_the_model_bit_for_bit(ctx, layout, n):
    thr, ref, off, cell, w = _dev()
    exp = expected(n)
    est, count = ctx.tumour_fraction(ctx.records(_pack(ctx, cohort(n), layout), layout, n), P, thr, ref, off, cell, w, cov=COV)
    assert est.shape == (n, len(off) - 1, 4) and count.shape == (n, len(off) - 1, 2)
    got = _got((est, count))
    assert np.array_equal(got[1], exp[1])
    diff = np.argwhere(bits(got[0]) != bits(exp[0]))
    assert len(diff) == 0, (diff[:8], got[0][tuple(diff[0])], exp[0][tuple(diff[0])])
    q, f, s = (got[0][:, l] for l in (LIST_QUIET, LIST_FULL, LIST_SILENT))
    assert (q[:, fm.F_HAT] == 0).all() and (q[:, fm.F_HI] > 0).all() and (f[:, fm.F_HAT] == 1).all() and (f[:, fm.F_HI] == 1).all() and (s[:, fm.F_HI] == 0).all()


@pytest.mark.parametrize("layout", ["i32", "u16"])
@pytest.mark.parametrize("kw", [dict(max_vaf_pm=250), dict(max_vaf_pm=0), dict(cov=0), dict(cov=3001), dict(z2=fm.Z2["0.90"]), dict(z2=fm.Z2["0.99"])])
def test_the_cap_the_cut_off_and_the_quantile(ctx, layout, kw):
    n = 9
    thr, ref, off, cell, w = _dev()
    exp = fm.fraction_model(cohort(n), P, panel()[0], panel()[1], off, cell, w, kw.get("cov", COV), kw.get("max_vaf_pm", 1000), kw.get("z2", fm.Z2_95))
    got = _got(ctx.tumour_fraction(ctx.records(_pack(ctx, cohort(n), layout), layout, n), P, thr, ref, off, cell, w, **{"cov": COV, **kw}))
    assert same(got, exp)
    if "max_vaf_pm" in kw:
        assert (got[0][:, LIST_FULL] == fm.NA).all()


@pytest.mark.parametrize("layout", ["i32", "u24", "u16"])
def test_a_padded_row_stride(ctx, layout):
    n, pad = 9, 7
    recs = np.concatenate([cohort(n), cohort(n)[:, 20:20 + pad]], axis=1)  # the pad holds records too: they must not be read in place of the next row's
    thr, ref, off, cell, w = _dev()
    got = _got(ctx.tumour_fraction(ctx.records(_pack(ctx, recs, layout), layout, n, row_stride=P + pad), P, thr, ref, off, cell, w, cov=COV))
    assert same(got, expected(n))


def test_i32_fields_of_two_to_the_thirty_and_the_largest(ctx):
    n = 9
    recs = big_records(P, n)
    thr, ref, off, cell, w = _dev()
    exp = fm.fraction_model(recs, P, panel()[0], panel()[1], off, cell, w, COV, 1000)
    assert (recs == 1 << 30).any() and (recs == (1 << 31) - 1).any() and (exp[1][:, :, fm.N_EVAL] > 0).any() and (exp[0][:, :, fm.F_HAT] > 0).any()
    assert same(_got(ctx.tumour_fraction(ctx.records(_t(recs), "i32", n), P, thr, ref, off, cell, w, cov=COV)), exp)


def test_offsets_beyond_W(ctx):
    """device lists are taken as they are: a list that runs over W is cut there, the ones behind it are empty"""
    n = 3
    thr, ref, off, cell, w = _dev()
    W = int(off[6]) + 10
    exp = fm.fraction_model(cohort(n), P, panel()[0], panel()[1], off, cell[:W], w[:W], COV, 1000)
    assert (exp[1][:, 7:] == 0).all() and (exp[1][:, 6, 0] > 0).any()
    d_off, d_cell, d_w = _t(off.astype(np.int32)), _t(cell[:W].astype(np.int32)), _t(w[:W])
    assert same(_got(ctx.tumour_fraction(ctx.records(_t(cohort(n)), "i32", n), P, thr, ref, d_off, d_cell, d_w, cov=COV)), exp)


@pytest.mark.parametrize("layout", ["i32", "u16"])
def test_chunks_into_the_rows_of_one_matrix_and_two_runs(ctx, layout):
    import torch

    n, cuts = 17, (0, 1, 9, 17)
    thr, ref, off, cell, w = _dev()
    L = len(off) - 1
    est = torch.full((n, L, 4), float("nan"), dtype=torch.float64, device=ctx.device)
    count = torch.full((n, L, 2), -1, dtype=torch.int64, device=ctx.device)
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        ctx.tumour_fraction(ctx.records(_pack(ctx, cohort(n)[lo:hi], layout), layout, hi - lo), P, thr, ref, off, cell, w, cov=COV, est=est[lo:hi], count=count[lo:hi])
    assert same(_got((est, count)), expected(n))
    rec = ctx.records(_pack(ctx, cohort(n), layout), layout, n)
    one, two = _got(ctx.tumour_fraction(rec, P, thr, ref, off, cell, w, cov=COV)), _got(ctx.tumour_fraction(rec, P, thr, ref, off, cell, w, cov=COV))
    assert one[0].tobytes() == two[0].tobytes() and one[1].tobytes() == two[1].tobytes()
