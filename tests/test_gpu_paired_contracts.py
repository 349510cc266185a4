"""The output contract C19 (include/amplisolve_hip.h) of ampli_pair_score_records on poisoned, fenced buffers (tests/helpers.py): d_s is
fully overwritten for n_pairs * P positions and nothing beyond them -- the other batches' pairs of a larger matrix included -- inputs
that end where their buffers end are unchanged, and every refusal comes with its code and leaves the outputs untouched."""
import ctypes as C

import numpy as np
import pytest

from amplisolve_amd._lib import Records
from tests.helpers import fenced
from tests.test_gpu_loo import _pack
from tests.test_gpu_paired import CUTOFF, NA, S_TOL, _case
from tests.test_gpu_parity import _t

pytestmark = pytest.mark.gpu
E_INVALID, E_RANGE = -1, -6


def _fenced_copy(t):
    buf, chk = fenced(tuple(t.shape), t.dtype)
    buf.copy_(t)
    return buf, chk


@pytest.mark.parametrize("layout", ["i32", "u24", "u16"])
@pytest.mark.parametrize("P,n_pairs,kind", [(1, 1, "same"), (65, 9, "different"), (130, 9, "same")])
def test_s_is_fully_overwritten_and_pairs_of_a_larger_matrix(ctx, layout, P, n_pairs, kind):
    import torch

    A, B, ref, pairs, want, want64 = _case(P, n_pairs, kind)
    # primary records only, so that the records end where their buffer ends: a row is P records
    src_a, chk_a = _fenced_copy(_pack(ctx, np.ascontiguousarray(A[0][:, :P]), layout))
    src_b, chk_b = _fenced_copy(_pack(ctx, np.ascontiguousarray(B[0][:, :P]), layout))
    ra, rb = ctx.records(src_a, layout, A[0].shape[0]), ctx.records(src_b, layout, B[0].shape[0])
    d_pairs, chk_p = _fenced_copy(_t(np.array(pairs, np.int32)))
    d_ref, chk_r = _fenced_copy(_t(ref))
    s, chk_s = fenced((n_pairs, P, 4, 2), torch.float32)
    checks = (chk_a, chk_b, chk_p, chk_r, chk_s)
    before = [t.clone() for t in (src_a, src_b, d_pairs, d_ref)]
    lo = n_pairs // 2
    ctx.pair_score(ra, rb, P, d_pairs[lo:], d_ref, CUTOFF, s=s[lo:])
    ctx.sync()
    [c() for c in checks]
    got = s.cpu().numpy()
    assert (got[:lo].view(np.uint32) == 0xFFFFFFFF).all()  # the other batch's pairs: untouched
    assert not np.isnan(got[lo:]).any()                     # over the poison: every cell written
    assert np.array_equal(got[lo:] == NA, want[lo:] == NA) and (np.abs(got[lo:].astype(np.float64) - want64[lo:]) <= S_TOL).all()
    if lo:
        ctx.pair_score(ra, rb, P, d_pairs[:lo], d_ref, CUTOFF, s=s[:lo])
    ctx.pair_score(ra, rb, P, d_pairs[lo:], d_ref, CUTOFF, s=s[lo:])  # again, over its own results
    ctx.sync()
    [c() for c in checks]
    got = s.cpu().numpy()
    assert np.array_equal(got == NA, want == NA) and np.array_equal(np.sign(got), np.sign(want))
    for t, b in zip((src_a, src_b, d_pairs, d_ref), before):
        assert torch.equal(t, b)  # the inputs are unchanged


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

    P, n_pairs = 65, 9
    A, B, ref, pairs, want, want64 = _case(P, n_pairs, "different")
    E = A[1]
    src = _t(A[0])
    src_b = _t(np.ascontiguousarray(B[0][:, :P]))
    ra = ctx.records(src, "i32", A[0].shape[0], row_stride=P + E)
    rb = ctx.records(src_b, "i32", B[0].shape[0])
    rb16 = ctx.records(_pack(ctx, np.ascontiguousarray(B[0][:, :P]), "u16"), "u16", B[0].shape[0])
    d_pairs, d_ref = _t(np.array(pairs, np.int32)), _t(ref)
    s, chk_s = fenced((n_pairs, P, 4, 2), torch.float32)
    L = ctx.lib

    def score(h=ctx.h, a=ra, b=rb, P_=P, pr=d_pairs, n=n_pairs, rf=d_ref, cut=CUTOFF, out=s):
        return L.ampli_pair_score_records(h, C.byref(a) if a is not None else None, C.byref(b) if b is not None else None, P_, _p(pr), n, _p(rf), cut, _p(out))

    bad = [score(h=None), score(a=None), score(b=None), score(a=_with(ra, recs=None)), score(b=_with(rb, recs=None)), score(P_=0), score(P_=-1), score(n=0),
           score(n=-3), score(cut=-1), score(pr=None), score(pr=_odd(d_pairs, 2)), score(rf=None), score(out=None), score(out=_odd(s, 4)), score(out=_odd(s, 8)),
           score(a=_with(ra, layout=3)), score(b=_with(rb, layout=-1)), score(a=_with(ra, n_samples=0)), score(b=_with(rb, n_samples=-2)),
           score(a=_with(ra, row_stride=P - 1)), score(b=_with(rb, row_stride=P - 1)), score(a=_with(ra, recs=src.data_ptr() + 4)),
           score(b=rb16), score(a=rb16, b=rb)]  # chunks of different layouts
    ctx.sync()
    assert bad == [E_INVALID] * len(bad), bad
    assert score(b=rb16) == E_INVALID and "layout" in L.ampli_last_error(ctx.h).decode()
    assert score(cut=-1) == E_INVALID and "depth_cutoff" in L.ampli_last_error(ctx.h).decode()
    # the range: nothing is launched, so the sizes need not be real
    for rc in (score(P_=(1 << 31) - 1, a=_with(ra, row_stride=0), b=_with(rb, row_stride=0)), score(P_=1 << 40, a=_with(ra, row_stride=0), b=_with(rb, row_stride=0))):
        assert rc == E_RANGE and "2^31" in L.ampli_last_error(ctx.h).decode()
    ctx.sync()
    chk_s()
    assert (chk_s.raw == 0xFF).all()  # nothing written, the payload included
    assert score() == 0 and score(a=rb16, b=rb16, pr=_t(np.array([[0, 1]] * n_pairs, np.int32))) == 0
    assert score() == 0
    ctx.sync()
    chk_s()
    got = s.cpu().numpy()
    assert np.array_equal(got == NA, want == NA) and (np.abs(got.astype(np.float64) - want64) <= S_TOL).all()
