"""The output contract C28 of ampli_fraction_records (include/amplisolve_hip.h) on poisoned, fenced buffers (tests/helpers.py): every
value and count of the call's rows written whatever the matrices held -- empty lists included, with plain stores: the other chunks' rows
of a larger matrix keep what they held -- and nothing written outside.  What is read ends where its buffer ends: records, thresholds,
reference codes, list_off of exactly L + 1 and list_cell and list_w of exactly W words."""
import ctypes as C

import numpy as np
import pytest

from amplisolve_amd._lib import FractionParams
from tests import fraction_model as fm
from tests.fraction_cases import COV, P, cohort, expected, lists, panel
from tests.helpers import fenced
from tests.test_fraction_host import same
from tests.test_gpu_loo import _pack
from tests.test_gpu_parity import _t

pytestmark = pytest.mark.gpu


def _fenced_copy(t):
    buf, chk = fenced(tuple(t.shape), t.dtype)
    buf.copy_(t)
    return buf, chk


def _inputs(ctx, recs, layout):
    """the read-only arguments, each in a fenced buffer of exactly its size"""
    import torch

    thr, ref = panel()
    off, cell, w = lists()
    assert int(cell[-1]) == 4 * P - 1 and int(off[-1]) == len(cell) == len(w)  # the last list's last entry is the last cell of the panel
    bufs = [_fenced_copy(x) for x in (_pack(ctx, recs, layout), _t(thr), _t(ref), _t(off.astype(np.int32)), _t(cell.astype(np.int32)), _t(w))]
    before = [b.clone() for b, _ in bufs]

    def unchanged():
        for (b, chk), was in zip(bufs, before):
            chk()
            assert torch.equal(b.view(torch.uint8), was.view(torch.uint8))

    return [b for b, _ in bufs], unchanged


@pytest.mark.parametrize("layout", ["i32", "u24", "u16"])
def test_a_chunks_rows_of_a_larger_matrix(ctx, layout):
    import torch

    n, total = 9, 12  # the chunk's rows lie inside a larger matrix
    exp = expected(n)
    L = exp[0].shape[1]
    (src, thr, ref, off, cell, w), unchanged = _inputs(ctx, cohort(n), layout)
    est, chk_e = fenced((total, L, 4), torch.float64)
    count, chk_c = fenced((total, L, 2), torch.int64)
    for _ in range(2):  # the second time over its own results
        ctx.tumour_fraction(ctx.records(src, layout, n), P, thr, ref, off, cell, w, cov=COV, est=est[2:2 + n], count=count[2:2 + n])
        ctx.sync()
        chk_e(), chk_c(), unchanged()
        got_e, got_c = est.cpu().numpy(), count.cpu().numpy()
        assert np.isnan(got_e[:2]).all() and np.isnan(got_e[2 + n:]).all() and (got_c[:2] == -1).all() and (got_c[2 + n:] == -1).all()  # not this call's
        assert same((got_e[2:2 + n], got_c[2:2 + n]), exp) and not np.isnan(got_e[2:2 + n]).any()  # every cell, the empty lists' NA too


def test_empty_lists_only_end_where_the_buffers_end(ctx):
    """W = 0: list_cell and list_w are valid pointers that are never read through; the last row's last list is the last bytes of both
    outputs"""
    import torch

    n, L = 8, 3
    thr, ref = panel()
    d_cell, chk_cell = fenced((1,), torch.int32)
    d_w, chk_w = fenced((1,), torch.float32)
    est, chk_e = fenced((n, L, 4), torch.float64)
    count, chk_c = fenced((n, L, 2), torch.int64)
    rec = ctx.records(_pack(ctx, cohort(n), "u16"), "u16", n)
    prm = FractionParams(COV, 1000, fm.Z2_95)
    d_off, d_thr, d_ref = _t(np.zeros(L + 1, np.int32)), _t(thr), _t(ref)
    assert ctx.lib.ampli_fraction_records(ctx.h, C.byref(rec), P, d_thr.data_ptr(), d_ref.data_ptr(), d_off.data_ptr(), d_cell.data_ptr(), d_w.data_ptr(), L, 0,
                                          C.byref(prm), est.data_ptr(), count.data_ptr()) == 0
    ctx.sync()
    chk_e(), chk_c(), chk_cell(), chk_w()
    assert (est.cpu().numpy() == fm.NA).all() and (count.cpu().numpy() == 0).all()
