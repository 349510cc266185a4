"""The refusals of ampli_dilute_records: each comes with its code before anything is launched and leaves the poison of the fenced
outputs whole (C21, include/amplisolve_hip.h)."""
import ctypes as C

import numpy as np
import pytest

from amplisolve_amd._lib import Records
from tests.dilution_cohorts import case
from tests.helpers import fenced
from tests.test_gpu_dilution_contracts import _descriptors
from tests.test_gpu_loo import _pack
from tests.test_gpu_parity import _t

pytestmark = pytest.mark.gpu
E_INVALID, E_RANGE = -1, -6


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

    P, n_mix = 65, 9
    A, B, mix, want, want_flags = case(P, n_mix, "different")
    E = A[1]
    src = _t(A[0])
    src_b = _t(np.ascontiguousarray(B[0][:, :P]))
    ra = ctx.records(src, "i32", A[0].shape[0], row_stride=P + E)
    rb = ctx.records(src_b, "i32", B[0].shape[0])
    rb16 = ctx.records(_pack(ctx, np.ascontiguousarray(B[0][:, :P]), "u16"), "u16", B[0].shape[0])
    d_mix = _t(_descriptors(mix))
    out, chk_o = fenced((n_mix, P, 8), torch.int32)
    flags, chk_f = fenced((n_mix,), torch.int32)
    L = ctx.lib

    def run(h=ctx.h, a=ra, b=rb, P_=P, mx=d_mix, n=n_mix, o=out, f=flags):
        return L.ampli_dilute_records(h, C.byref(a) if a is not None else None, C.byref(b) if b is not None else None, P_, _p(mx), n, _p(o), _p(f))

    bad = [run(h=None), run(a=None), run(a=_with(ra, recs=None)), run(b=_with(rb, recs=None)), run(P_=0), run(P_=-1), run(n=0), run(n=-3), run(mx=None),
           run(mx=_odd(d_mix, 4)), run(o=None), run(o=_odd(out, 4)), run(o=_odd(out, 8)), run(f=None), run(f=_odd(flags, 2)),
           run(a=_with(ra, layout=3)), run(b=_with(rb, layout=-1)), run(a=_with(ra, n_samples=0)), run(b=_with(rb, n_samples=-2)),
           run(a=_with(ra, row_stride=P - 1)), run(b=_with(rb, row_stride=P - 1)), run(a=_with(ra, recs=src.data_ptr() + 4)),
           run(b=_with(rb, recs=src_b.data_ptr() + 8))]
    ctx.sync()
    assert bad == [E_INVALID] * len(bad), bad
    assert run(f=None) == E_INVALID and "d_flags" in L.ampli_last_error(ctx.h).decode()
    # the range: nothing is launched, so the sizes need not be real
    for rc in (run(P_=(1 << 31) - 1, a=_with(ra, row_stride=0), b=_with(rb, row_stride=0)), run(P_=1 << 40, a=_with(ra, row_stride=0), b=_with(rb, row_stride=0))):
        assert rc == E_RANGE and "2^31" in L.ampli_last_error(ctx.h).decode()
    ctx.sync()
    chk_o()
    chk_f()
    assert (chk_o.raw == 0xFF).all() and (chk_f.raw == 0xFF).all()  # nothing written, the payloads included
    # chunks of different layouts are no refusal, and neither is a missing chunk b: its mixtures are bad mixtures
    assert run(b=rb16) == 0
    ctx.sync()
    assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(flags.cpu().numpy(), want_flags)
    assert run(b=None) == 0
    ctx.sync()
    named = np.array([m[1] >= 0 for m in mix])
    got, gf = out.cpu().numpy(), flags.cpu().numpy()
    assert (gf[named] == 2).all() and not gf[~named].any() and np.array_equal(got[~named], want[~named]) and (got[named][:, :, 0] == np.iinfo(np.int32).min).all()
    chk_o()
    chk_f()
