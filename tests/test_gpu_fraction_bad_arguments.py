"""Every refusal of ampli_fraction_records (include/amplisolve_hip.h) returns its code with both outputs untouched: poisoned, fenced
buffers (tests/helpers.py) keep every byte.  The same arguments, unbroken, then succeed."""
import ctypes as C

import numpy as np
import pytest

from amplisolve_amd._lib import FractionParams, Records
from tests import fraction_model as fm
from tests.fraction_cases import COV, P, cohort, lists, panel
from tests.helpers import fenced
from tests.test_gpu_parity import _t

pytestmark = pytest.mark.gpu
INVALID, RANGE = -1, -6


def test_every_refusal_leaves_the_outputs_untouched(ctx):
    import torch

    n = 3
    off, cell, w = lists()
    L, W = len(off) - 1, len(cell)
    recs = _t(cohort(n))
    rec = ctx.records(recs, "i32", n)
    thr, ref = panel()
    d = dict(thr=_t(thr), ref=_t(ref), off=_t(off.astype(np.int32)), cell=_t(cell.astype(np.int32)), w=_t(w))
    est, chk_e = fenced((n, L, 4), torch.float64)
    count, chk_c = fenced((n, L, 2), torch.int64)
    p = lambda t: t.data_ptr() if t is not None else None
    ok = FractionParams(COV, 1000, fm.Z2_95)

    def f_(h=ctx.h, r=rec, P_=P, thr_=d["thr"], ref_=d["ref"], off_=d["off"], cell_=d["cell"], w_=d["w"], L_=L, W_=W, prm=ok, est_=est, count_=count, est_by=0,
           count_by=0):
        return ctx.lib.ampli_fraction_records(h, C.byref(r) if r is not None else None, P_, p(thr_), p(ref_), p(off_), p(cell_), p(w_), L_, W_,
                                              C.byref(prm) if prm is not None else None, (p(est_) or 0) + est_by or None, (p(count_) or 0) + count_by or None)

    def odd(t):
        """the tensor's address two bytes on: not 4-byte aligned"""
        class _P:
            def data_ptr(self, a=t.data_ptr() + 2):
                return a
        return _P()

    assert f_(L_=0) == 0  # no list: nothing to write
    broken = ctx.records(recs, "i32", 0)
    short = ctx.records(recs, "i32", n, row_stride=P - 1)
    invalid = [f_(h=None), f_(r=None), f_(P_=0), f_(P_=-3), f_(thr_=None), f_(ref_=None), f_(off_=None), f_(cell_=None), f_(w_=None), f_(L_=-1), f_(W_=-1),
               f_(prm=None), f_(prm=FractionParams(-1, 1000, fm.Z2_95)), f_(prm=FractionParams(COV, -1, fm.Z2_95)), f_(prm=FractionParams(COV, 1001, fm.Z2_95)),
               f_(prm=FractionParams(COV, 1000, 0.0)), f_(prm=FractionParams(COV, 1000, -3.84)), f_(prm=FractionParams(COV, 1000, float("nan"))),
               f_(prm=FractionParams(COV, 1000, float("inf"))), f_(est_=None), f_(count_=None), f_(est_by=4), f_(count_by=4), f_(r=broken), f_(r=short),
               f_(thr_=odd(d["thr"])), f_(off_=odd(d["off"])), f_(cell_=odd(d["cell"])), f_(w_=odd(d["w"]))]
    assert all(rc == INVALID for rc in invalid), invalid
    many = Records.from_buffer_copy(rec)
    many.n_samples = 2097121  # refused before anything is launched: nothing that large is allocated
    ranged = [f_(r=many), f_(P_=(1 << 31) - 1), f_(W_=1 << 28)]
    assert all(rc == RANGE for rc in ranged), ranged
    ctx.sync()
    chk_e(), chk_c()
    for t in (est, count):
        assert (t.view(torch.uint8) == 0xFF).all()  # nothing was written
    assert b"fraction" in ctx.lib.ampli_last_error(ctx.h)
    assert f_() == 0  # the same arguments, unbroken
    ctx.sync()
    chk_e(), chk_c()
    assert not np.isnan(est.cpu().numpy()).any() and (count.cpu().numpy() >= 0).all()
