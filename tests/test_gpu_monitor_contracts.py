"""The output contracts C22-C24 of the monitoring entry points (include/amplisolve_hip.h) on poisoned, fenced buffers (tests/helpers.py):
every cell of the call's rows written whatever the matrices held -- empty lists and out-of-range pairs included, with plain stores: the
other chunks' rows keep what they held -- and nothing written outside.  What is read ends where its buffer ends: records, thresholds,
reference codes, list_off of exactly L + 1 and list_cell of exactly W words, cand_off of 5 and cand_pos of n_cand words.  Every refusal
leaves the outputs untouched."""
import ctypes as C

import numpy as np
import pytest

from amplisolve_amd._lib import MonitorParams, Records
from tests.helpers import fenced
from tests.monitor_cases import CONTROL_SEED, COV, cohort, control_case, expected, lists, panel
from tests.test_gpu_loo import _pack
from tests.test_gpu_parity import _t
from tests.test_monitor_host import bits, host_score

pytestmark = pytest.mark.gpu
INVALID, RANGE = -1, -6


def _fenced_copy(t):
    buf, chk = fenced(tuple(t.shape), t.dtype)
    buf.copy_(t)
    return buf, chk


def _inputs(ctx, P, recs, layout):
    """the read-only arguments, each in a fenced buffer of exactly its size"""
    import torch

    thr, ref = panel(P)
    off, cell = lists(P)
    assert int(cell[-1]) == 4 * P - 1 and int(off[-1]) == len(cell)  # the last list's last entry is the last cell of the panel
    bufs = [_fenced_copy(x) for x in (_pack(ctx, recs, layout), _t(thr), _t(ref), _t(off.astype(np.int32)), _t(cell.astype(np.int32)))]
    before = [b.clone() for b, _ in bufs]

    def unchanged():
        for (b, chk), was in zip(bufs, before):
            chk()
            assert torch.equal(b.view(torch.uint8), was.view(torch.uint8))

    return [b for b, _ in bufs], unchanged


@pytest.mark.parametrize("layout", ["i32", "u24", "u16"])
@pytest.mark.parametrize("P", [65, 1000])
def test_sums_of_a_chunk(ctx, layout, P):
    import torch

    n, lo, hi = 9, 0, 9
    total = 12  # the chunk's rows lie inside a larger matrix
    exp = expected(P, n)
    L = exp[0].shape[1]
    (src, thr, ref, off, cell), unchanged = _inputs(ctx, P, cohort(P, n), layout)
    sums, chk_s = fenced((total, L, 6), torch.int64)
    lam, chk_l = fenced((total, L, 2), torch.float64)
    ctx.monitor_sums(ctx.records(src, layout, n), P, thr, ref, off, cell, cov=COV, sums=sums[2:2 + n], lam=lam[2:2 + n])
    ctx.sync()
    chk_s(), chk_l(), unchanged()
    got_s, got_l = sums.cpu().numpy(), lam.cpu().numpy()
    assert (got_s[:2] == -1).all() and (got_s[2 + n:] == -1).all() and np.isnan(got_l[:2]).all() and np.isnan(got_l[2 + n:]).all()  # not this call's
    assert np.array_equal(got_s[2:2 + n], exp[0]) and np.array_equal(bits(got_l[2:2 + n]), bits(exp[1]))  # every cell, the empty lists' zeros too
    ctx.monitor_sums(ctx.records(src, layout, n), P, thr, ref, off, cell, cov=COV, sums=sums[2:2 + n], lam=lam[2:2 + n])  # again, over its own results
    ctx.sync()
    chk_s(), chk_l()
    assert np.array_equal(sums.cpu().numpy()[2:2 + n], exp[0])


def test_empty_lists_only_end_where_the_buffers_end(ctx):
    """W = 0: list_cell is a valid pointer that is never read through; the last row's last list is the last bytes of both payloads"""
    import torch

    P, n, L = 65, 8, 3
    thr, ref = panel(P)
    d_cell, chk_cell = fenced((1,), torch.int32)
    sums, chk_s = fenced((n, L, 6), torch.int64)
    lam, chk_l = fenced((n, L, 2), torch.float64)
    rec = ctx.records(_pack(ctx, cohort(P, n), "u16"), "u16", n)
    prm = MonitorParams(COV, 1000)
    d_off, d_thr, d_ref = _t(np.zeros(L + 1, np.int32)), _t(thr), _t(ref)
    assert ctx.lib.ampli_monitor_sums_records(ctx.h, C.byref(rec), P, d_thr.data_ptr(), d_ref.data_ptr(), d_off.data_ptr(), d_cell.data_ptr(), L, 0,
                                              C.byref(prm), sums.data_ptr(), lam.data_ptr()) == 0
    ctx.sync()
    chk_s(), chk_l(), chk_cell()
    assert (sums.cpu().numpy() == 0).all() and (bits(lam.cpu().numpy()) == 0).all()


@pytest.mark.parametrize("layout", ["i32", "u16"])
def test_controls(ctx, layout):
    import torch

    P, n, R = 65, 3, 7
    pairs, cand_off, cand_pos, exp_s, exp_l = control_case(P, n, R=R, first_rep=2)
    (src, thr, ref, off, cell), unchanged = _inputs(ctx, P, cohort(P, n), layout)
    d_pairs, chk_p = _fenced_copy(_t(pairs))
    d_co, chk_co = _fenced_copy(_t(cand_off.astype(np.int32)))
    d_cp, chk_cp = _fenced_copy(_t(cand_pos.astype(np.int32)))
    sums, chk_s = fenced(exp_s.shape, torch.int64)
    lam, chk_l = fenced(exp_l.shape, torch.float64)
    ctx.monitor_controls(ctx.records(src, layout, n), P, thr, ref, off, cell, d_pairs, d_co, d_cp, R, first_rep=2, seed=CONTROL_SEED, cov=COV, sums=sums, lam=lam)
    ctx.sync()
    for c in (chk_s, chk_l, chk_p, chk_co, chk_cp, unchanged):
        c()
    assert np.array_equal(sums.cpu().numpy(), exp_s) and np.array_equal(bits(lam.cpu().numpy()), bits(exp_l))  # the zeros of the bad pairs too
    assert np.array_equal(d_pairs.cpu().numpy(), pairs) and np.array_equal(d_cp.cpu().numpy().view(np.uint32), cand_pos)


@pytest.mark.parametrize("n_cells", [1, 65, 1000])
def test_scores(ctx, n_cells):
    import torch

    rng = np.random.default_rng(n_cells)
    s = rng.integers(0, 40, (n_cells, 6)).astype(np.int64)
    l = np.exp(rng.uniform(np.log(1e-3), np.log(1e3), (n_cells, 2)))
    d_s, chk_s = _fenced_copy(_t(s))
    d_l, chk_l = _fenced_copy(_t(l))
    q, chk_q = fenced((n_cells, 2), torch.float32)
    ctx.monitor_score(d_s, d_l, q=q)
    ctx.sync()
    chk_s(), chk_l(), chk_q()
    got = q.cpu().numpy()
    assert not np.isnan(got).any() and np.array_equal(got.view(np.int32), host_score(s, l).view(np.int32))
    assert np.array_equal(d_s.cpu().numpy(), s) and np.array_equal(bits(d_l.cpu().numpy()), bits(l))


def test_every_refusal_leaves_the_outputs_untouched(ctx):
    import torch

    P, n, R = 65, 3, 2
    off, cell = lists(P)
    L, W = len(off) - 1, len(cell)
    pairs, cand_off, cand_pos, _, _ = control_case(P, n, R=R)
    recs = _t(cohort(P, n))
    rec = ctx.records(recs, "i32", n)
    thr, ref = panel(P)
    d = dict(thr=_t(thr), ref=_t(ref), off=_t(off.astype(np.int32)), cell=_t(cell.astype(np.int32)), pairs=_t(pairs), co=_t(cand_off.astype(np.int32)),
             cp=_t(cand_pos.astype(np.int32)))
    sums, chk_s = fenced((max(n, len(pairs)), max(L, R), 6), torch.int64)
    lam, chk_l = fenced((max(n, len(pairs)), max(L, R), 2), torch.float64)
    q, chk_q = fenced((16, 2), torch.float32)
    p = lambda t: t.data_ptr() if t is not None else None
    lib = ctx.lib
    ok = MonitorParams(COV, 1000)

    def s_(h=ctx.h, r=rec, P_=P, thr_=d["thr"], ref_=d["ref"], off_=d["off"], cell_=d["cell"], L_=L, W_=W, prm=ok, out=sums, lam_=lam, off_by=0, lam_by=0):
        return lib.ampli_monitor_sums_records(h, C.byref(r) if r is not None else None, P_, p(thr_), p(ref_), p(off_), p(cell_), L_, W_,
                                              C.byref(prm) if prm is not None else None, (p(out) or 0) + off_by or None, (p(lam_) or 0) + lam_by or None)

    def c_(h=ctx.h, r=rec, P_=P, thr_=d["thr"], L_=L, W_=W, pairs_=d["pairs"], np_=len(pairs), co=d["co"], cp=d["cp"], nc=len(cand_pos), R_=R, first=0, prm=ok,
           out=sums, lam_=lam):
        return lib.ampli_monitor_control_records(h, C.byref(r) if r is not None else None, P_, p(thr_), p(d["ref"]), p(d["off"]), p(d["cell"]), L_, W_, p(pairs_),
                                                 np_, p(co), p(cp), nc, R_, first, 7, C.byref(prm) if prm is not None else None, p(out), p(lam_))

    def odd(t):
        """the tensor's address two bytes on: not 4-byte aligned"""
        class _P:
            def data_ptr(self, a=t.data_ptr() + 2):
                return a
        return _P()

    def q_(h=ctx.h, s=sums, l=lam, n_=16, out=q, by=0):
        return lib.ampli_monitor_score(h, p(s), p(l), n_, (p(out) or 0) + by or None)

    broken = ctx.records(recs, "i32", 0)
    short = ctx.records(recs, "i32", n, row_stride=P - 1)
    invalid = [s_(h=None), s_(r=None), s_(P_=0), s_(P_=-3), s_(thr_=None), s_(ref_=None), s_(off_=None), s_(cell_=None), s_(L_=0), s_(W_=-1), s_(prm=None),
               s_(prm=MonitorParams(-1, 1000)), s_(prm=MonitorParams(COV, -1)), s_(prm=MonitorParams(COV, 1001)), s_(out=None), s_(lam_=None), s_(off_by=4),
               s_(lam_by=4), s_(r=broken), s_(r=short),
               c_(h=None), c_(r=None), c_(P_=0), c_(thr_=None), c_(L_=0), c_(W_=-1), c_(pairs_=None), c_(np_=0), c_(co=None), c_(cp=None), c_(nc=-1), c_(R_=0),
               c_(first=-1), c_(prm=None), c_(prm=MonitorParams(COV, 1001)), c_(out=None), c_(lam_=None), c_(r=broken),
               s_(thr_=odd(d["thr"])), s_(off_=odd(d["off"])), s_(cell_=odd(d["cell"])), c_(thr_=odd(d["thr"])), c_(pairs_=odd(d["pairs"])), c_(co=odd(d["co"])),
               c_(cp=odd(d["cp"])),
               q_(h=None), q_(s=None), q_(l=None), q_(n_=0), q_(out=None), q_(by=4)]
    assert all(rc == INVALID for rc in invalid), invalid
    many = Records.from_buffer_copy(rec)
    many.n_samples = 2097121  # refused before anything is launched: nothing that large is allocated
    ranged = [s_(r=many), s_(P_=(1 << 31) - 1), s_(W_=1 << 28), c_(P_=(1 << 31) - 1), c_(W_=1 << 28), c_(nc=1 << 32), c_(first=(1 << 31) - 2)]
    assert all(rc == RANGE for rc in ranged), ranged
    ctx.sync()
    chk_s(), chk_l(), chk_q()
    for t in (sums, lam, q):
        assert (t.view(torch.uint8) == 0xFF).all()  # nothing was written
    assert b"monitor" in ctx.lib.ampli_last_error(ctx.h)
    assert s_() == 0 and c_() == 0 and q_() == 0  # the same arguments, unbroken
    ctx.sync()
    chk_s(), chk_l(), chk_q()
    assert not np.isnan(q.cpu().numpy()).any()
