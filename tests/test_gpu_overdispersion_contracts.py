"""The output contract C18 (include/amplisolve_hip.h) of ampli_overdispersion_records, ampli_overdispersion_finalize and
ampli_nb_score_records on poisoned, fenced buffers (tests/helpers.py) -- overwrite, then accumulate, then overwrite; the rows of a larger
matrix; inputs that end where their buffers end -- and every refusal with its code, the outputs untouched."""
import ctypes as C

import numpy as np
import pytest

from amplisolve_amd._lib import Records
from tests.helpers import fenced
from tests.overdispersion_model import s2_model
from tests.test_gpu_loo import _pack
from tests.test_gpu_overdispersion import CUTOFF, NA, _q_case, _s2_case
from tests.test_gpu_parity import _t

pytestmark = pytest.mark.gpu
E_INVALID, E_RANGE = -1, -6


def _fenced_copy(t):
    buf, chk = fenced(tuple(t.shape), t.dtype)
    buf.copy_(t)
    return buf, chk


@pytest.mark.parametrize("layout", ["i32", "u24", "u16"])
@pytest.mark.parametrize("P,n", [(1, 1), (65, 5), (130, 9)])
def test_s2_overwrite_accumulate_overwrite(ctx, layout, P, n):
    import torch

    (recs, E, dup_off, ext_pos, _), exp = _s2_case(P, n)
    cut = max(1, n // 2)
    first = s2_model(recs[:cut], P, 30, E=E, ext_pos=ext_pos).astype(np.float64)
    parts = (recs[:cut], recs[cut:]) if n > 1 else (recs,)
    srcs = [_fenced_copy(_pack(ctx, part, layout)) for part in parts]  # the records end where their buffers end
    d_dup, chk_dup = _fenced_copy(_t(dup_off))
    ch = [ctx.records(src, layout, len(part), E=E, dup_off=d_dup, ext_pos=_t(ext_pos)) for (src, _), part in zip(srcs, parts)]
    s2, chk = fenced((2, 4, P), torch.float64)
    acc0 = ctx.new_acc(P)
    checks = [chk, chk_dup] + [c for _, c in srcs]
    ctx.overdispersion_sums(ch[0], P, acc0, 30, s2=s2)
    ctx.sync()
    [c() for c in checks]
    assert np.array_equal(s2.cpu().numpy(), first if n > 1 else exp.astype(np.float64))  # over the poison: every cell written
    if n > 1:
        ctx.overdispersion_sums(ch[1], P, acc0, 30, s2=s2, accumulate=True)
        ctx.sync()
        [c() for c in checks]
        assert np.array_equal(s2.cpu().numpy(), exp.astype(np.float64))
    ctx.overdispersion_sums(ch[0], P, acc0, 30, s2=s2)  # again, over its own results
    ctx.sync()
    [c() for c in checks]
    assert np.array_equal(s2.cpu().numpy(), first if n > 1 else exp.astype(np.float64))


def test_omega_is_fully_overwritten(ctx):
    import torch

    P = 65
    rng = np.random.default_rng(2)
    x2, chk_x = _fenced_copy(_t(rng.uniform(0, 90, (2, 4, P))))
    s2v, chk_s = _fenced_copy(_t(rng.uniform(1e6, 5e7, (2, 4, P))))
    st, chk_st = _fenced_copy(_t(rng.choice(np.array([0, 1, 0x40], np.uint8), (2, 4, P))))
    omega, chk_w = fenced((2, 4, P), torch.float64)
    acc0 = ctx.new_acc(P)
    acc0.snt.copy_(_t(rng.integers(2, 50, (2, 4, P)).astype(np.float64)))
    acc0.srd.copy_(_t(rng.integers(9000, 20000, (2, 4, P))))
    acc0.cnt.copy_(_t(rng.integers(2, 9, (4, P)).astype(np.int32)))
    ctx.overdispersion_fit(P, acc0, x2, s2v, st, omega=omega)
    ctx.sync()
    [c() for c in (chk_x, chk_s, chk_st, chk_w)]
    w = omega.cpu().numpy()
    high = (st.cpu().numpy() & 0x40) != 0
    assert np.isfinite(w).all() and (w[~high] == 0).all() and (w >= 0).all() and (w[high] > 0).any()


@pytest.mark.parametrize("layout", ["i32", "u24", "u16"])
@pytest.mark.parametrize("P,n_t", [(1, 1), (65, 9), (130, 5)])
def test_q_is_fully_overwritten_and_rows_of_a_larger_matrix(ctx, layout, P, n_t):
    import torch

    recs, ref, thr, omega, _, q_m, _ = _q_case(P, n_t)
    lo = n_t // 2
    src_a, chk_a = _fenced_copy(_pack(ctx, recs[lo:], layout))  # the records end where their buffer ends
    d_thr, chk_t = _fenced_copy(_t(thr))
    d_w, chk_w = _fenced_copy(_t(omega))
    d_ref, chk_r = _fenced_copy(_t(ref))
    q, chk_q = fenced((n_t, P, 4, 2), torch.float32)
    checks = (chk_a, chk_t, chk_w, chk_r, chk_q)
    ctx.nb_score(ctx.records(src_a, layout, n_t - lo), P, d_thr, d_ref, d_w, CUTOFF, q=q[lo:])
    ctx.sync()
    [c() for c in checks]
    got = q.cpu().numpy()
    assert (got[:lo].view(np.uint32) == 0xFFFFFFFF).all()  # the other chunk's rows: untouched
    assert np.array_equal(got[lo:] == NA, q_m[lo:] == NA) and (np.abs(got[lo:].astype(np.float64) - q_m[lo:]) <= 1e-5).all()
    if lo:
        ctx.nb_score(ctx.records(_pack(ctx, recs[:lo], layout), layout, lo), P, d_thr, d_ref, d_w, CUTOFF, q=q[:lo])
    ctx.nb_score(ctx.records(src_a, layout, n_t - lo), P, d_thr, d_ref, d_w, CUTOFF, q=q[lo:])  # again, over its own results
    ctx.sync()
    [c() for c in checks]
    got = q.cpu().numpy()
    assert np.array_equal(got == NA, q_m == NA) and (np.abs(got.astype(np.float64) - q_m) <= 1e-5).all()


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _odd(t, k):
    import torch

    return t.view(torch.uint8).reshape(-1)[k:]


def _with(base, **kw):
    r = Records.from_buffer_copy(base)
    for k, v in kw.items():
        setattr(r, k, v)
    return r


def test_refusals(ctx):
    import torch

    P, n = 65, 5
    (recs, E, dup_off, ext_pos, _), _ = _s2_case(P, n)
    src = _t(recs)
    rec = ctx.records(src, "i32", n, E=E, dup_off=_t(dup_off), ext_pos=_t(ext_pos))
    trec = ctx.records(src, "i32", n, row_stride=P + E)
    acc0, acc_other = ctx.new_acc(P), ctx.new_acc(P + 1)
    s2, chk_s = fenced((2, 4, P), torch.float64)
    omega, chk_w = fenced((2, 4, P), torch.float64)
    q, chk_q = fenced((n, P, 4, 2), torch.float32)
    x2 = _t(np.ones((2, 4, P)))
    st = _t(np.full((2, 4, P), 0x40, np.uint8))
    thr = _t(np.full((2, 4, P), 0.002, np.float32))
    ref = _t(np.zeros(P, np.uint8))
    L = ctx.lib

    def sums(h=ctx.h, r=rec, P_=P, a=acc0, cov=30, out=s2, acc=0):
        return L.ampli_overdispersion_records(h, C.byref(r) if r is not None else None, P_, C.byref(a.struct) if a is not None else None, cov, _p(out), acc)

    def fit(h=ctx.h, P_=P, a=acc0, x=x2, s=s2, st_=st, w=omega):
        return L.ampli_overdispersion_finalize(h, P_, C.byref(a.struct) if a is not None else None, _p(x), _p(s), _p(st_), _p(w))

    def score(h=ctx.h, r=trec, P_=P, t=thr, w=None, rf=ref, cut=100, out=q):
        return L.ampli_nb_score_records(h, C.byref(r) if r is not None else None, P_, _p(t), _p(w), _p(rf), cut, _p(out))

    bad = [sums(h=None), sums(r=None), sums(r=_with(rec, recs=None)), sums(P_=0), sums(P_=-1), sums(cov=0), sums(cov=-5), sums(out=None),
           sums(out=_odd(s2, 4)), sums(a=None), sums(a=acc_other), sums(r=_with(rec, layout=3)), sums(r=_with(rec, n_samples=0)),
           sums(r=_with(rec, dup_off=None)), sums(r=_with(rec, row_stride=P + E - 1)), sums(r=_with(rec, recs=src.data_ptr() + 4)), sums(acc=1, out=None),
           fit(h=None), fit(P_=0), fit(a=None), fit(a=acc_other), fit(x=None), fit(s=None), fit(st_=None), fit(w=None), fit(w=_odd(omega, 4)),
           fit(x=_odd(x2, 4)),
           score(h=None), score(r=None), score(r=_with(trec, recs=None)), score(P_=0), score(cut=-1), score(t=None), score(rf=None), score(out=None),
           score(out=_odd(q, 4)), score(out=_odd(q, 8)), score(t=_odd(thr, 2)), score(w=_odd(omega, 4)), score(r=_with(trec, layout=-1)),
           score(r=_with(trec, n_samples=0)), score(r=_with(trec, n_samples=-2)), score(r=_with(trec, row_stride=P - 1)),
           score(r=_with(trec, recs=src.data_ptr() + 4))]
    ctx.sync()
    assert bad == [E_INVALID] * len(bad), bad
    assert score(cut=-1) == E_INVALID and "calling_cutoff" in L.ampli_last_error(ctx.h).decode()
    # the range: nothing is launched, so the sizes need not be real
    for rc in (sums(P_=(1 << 31) - 1), fit(P_=(1 << 31) - 1), score(P_=(1 << 31) - 1, r=_with(trec, row_stride=0)), score(P_=1 << 40, r=_with(trec, row_stride=0))):
        assert rc == E_RANGE and "2^31" in L.ampli_last_error(ctx.h).decode()
    ctx.sync()
    for chk in (chk_s, chk_w, chk_q):
        chk()
        assert (chk.raw == 0xFF).all()  # nothing written, the payloads included
    assert sums() == 0 and fit() == 0 and score(cut=0) == 0
    ctx.sync()
    [chk() for chk in (chk_s, chk_w, chk_q)]
    assert np.array_equal(s2.cpu().numpy(), s2_model(recs, P, 30, E=E, ext_pos=ext_pos).astype(np.float64))
    assert np.isfinite(q.cpu().numpy()).all() and not (chk_w.raw == 0xFF).all()  # omega of an unreduced table means nothing, but it is written
