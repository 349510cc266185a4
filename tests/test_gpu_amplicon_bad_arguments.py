"""The amplicon entry points refuse bad arguments -- AMPLI_E_INVALID for null or misaligned pointers, n <= 0, A <= 0, P <= 0, W < 0, a
negative cut-off, min_normals < 1 and broken records; AMPLI_E_RANGE, with a message that says so, for W >= 2^28, P >= 2^31 and N or A
above AMPLI_AMPLICON_MAX -- before anything is launched: every output, poisoned and fenced, stays untouched."""
import ctypes as C

import numpy as np
import pytest

from amplisolve_amd._lib import Records
from amplisolve_amd.api import AMPLICON_MAX
from tests.amplicon_model import depth_sums, ratios, reference, same
from tests.concordance_cohorts import records
from tests.helpers import fenced
from tests.test_gpu_amplicon import lists, matrix
from tests.test_gpu_parity import _t

pytestmark = pytest.mark.gpu
E_INVALID, E_RANGE = -1, -6
P, N = 65, 4


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _odd(t, k):
    import torch

    return t.view(torch.uint8).reshape(-1)[k:]


def test_depth_refusals(ctx):
    import torch

    recs = records(P, N, 5)
    off, pos = lists(P)
    A, W = len(off) - 1, len(pos)
    src = _t(recs)
    rec = ctx.records(src, "i32", N)
    rec16 = ctx.records(ctx.pack(src, "u16")[0], "u16", N)
    d_off, d_pos = _t(off.astype(np.int32)), _t(pos.astype(np.int32))
    out, chk = fenced((N, A, 4), torch.int64)
    L = ctx.lib

    def call(h=ctx.h, r=rec, P_=P, A_=A, o_=d_off, p_=d_pos, W_=W, cov=100, out_=out):
        return L.ampli_amplicon_depth_records(h, C.byref(r) if r is not None else None, P_, A_, _p(o_), _p(p_), W_, cov, _p(out_))

    def with_(base=rec, **kw):
        r = Records.from_buffer_copy(base)
        for k, v in kw.items():
            setattr(r, k, v)
        return r

    bad = [call(h=None), call(r=None), call(r=with_(recs=None)), call(P_=0), call(P_=-1), call(A_=0), call(A_=-2), call(W_=-1), call(cov=-1),
           call(r=with_(n_samples=0)), call(r=with_(n_samples=-3)), call(r=with_(layout=3)), call(r=with_(layout=-1)), call(r=with_(E=-1)),
           call(o_=None), call(p_=None), call(out_=None), call(o_=_odd(d_off, 2)), call(p_=_odd(d_pos, 1)), call(out_=_odd(out, 4)), call(out_=_odd(out, 1)),
           call(r=with_(row_stride=P - 1)), call(r=with_(recs=src.data_ptr() + 4))]
    ctx.sync()
    assert bad == [E_INVALID] * len(bad), bad
    assert L.ampli_last_error(ctx.h).decode() != ""
    # the ranges: nothing is launched, so the sizes need not be real
    assert call(W_=1 << 28) == E_RANGE
    msg = L.ampli_last_error(ctx.h).decode()
    assert "2^28" in msg and "W" in msg
    assert call(W_=1 << 40, r=rec16) == E_RANGE and "2^28" in L.ampli_last_error(ctx.h).decode()
    assert call(P_=(1 << 31) - 1) == E_RANGE and "2^31" in L.ampli_last_error(ctx.h).decode()
    assert call(P_=1 << 40, r=rec16) == E_RANGE
    assert call(r=with_(n_samples=2097121)) == E_RANGE and "n_samples" in L.ampli_last_error(ctx.h).decode()
    ctx.sync()
    chk()
    assert (chk.raw == 0xFF).all()  # nothing written, the payload included
    assert call() == 0
    ctx.sync()
    chk()
    assert np.array_equal(out.cpu().numpy(), depth_sums(recs, off, pos))
    assert call(r=rec16, cov=0) == 0  # the other layout, a cut-off of zero
    ctx.sync()
    assert np.array_equal(out.cpu().numpy(), depth_sums(recs, off, pos, 0))


def test_reference_and_ratio_refusals(ctx):
    import torch

    Nn, A = 5, 7
    sums, use = matrix(Nn, A)
    d_sums, d_use = _t(sums), _t(use)
    outs = {k: fenced(s, d) for k, (s, d) in dict(total=((Nn,), torch.int64), ref=((A, 2), torch.float64), status=((A,), torch.uint8),
                                                  centre=((Nn,), torch.float64), k=((Nn,), torch.int32), ratio=((Nn, A), torch.float64),
                                                  z=((Nn, A), torch.float64)).items()}
    o = {k: v[0] for k, v in outs.items()}
    good_ref, good_status = _t(np.ones((A, 2))), _t(np.zeros(A, np.uint8))
    L = ctx.lib

    def reference_(h=ctx.h, s=d_sums, N_=Nn, A_=A, u=d_use, mn=2, t=o["total"], r=o["ref"], st=o["status"]):
        return L.ampli_amplicon_reference(h, _p(s), N_, A_, _p(u), mn, _p(t), _p(r), _p(st))

    def ratio_(h=ctx.h, s=d_sums, S_=Nn, A_=A, u=d_use, r=good_ref, st=good_status, t=o["total"], c=o["centre"], k=o["k"], ra=o["ratio"], z=o["z"]):
        return L.ampli_amplicon_ratio(h, _p(s), S_, A_, _p(u), _p(r), _p(st), _p(t), _p(c), _p(k), _p(ra), _p(z))

    bad = [reference_(h=None), reference_(s=None), reference_(u=None), reference_(t=None), reference_(r=None), reference_(st=None), reference_(N_=0),
           reference_(N_=-1), reference_(A_=0), reference_(A_=-5), reference_(mn=0), reference_(mn=-1), reference_(s=_odd(d_sums, 4)),
           reference_(t=_odd(o["total"], 4)), reference_(r=_odd(o["ref"], 4)),
           ratio_(h=None), ratio_(s=None), ratio_(u=None), ratio_(r=None), ratio_(st=None), ratio_(t=None), ratio_(c=None), ratio_(k=None), ratio_(ra=None),
           ratio_(z=None), ratio_(S_=0), ratio_(S_=-1), ratio_(A_=0), ratio_(A_=-1), ratio_(s=_odd(d_sums, 4)), ratio_(r=_odd(good_ref, 4)),
           ratio_(t=_odd(o["total"], 4)), ratio_(c=_odd(o["centre"], 4)), ratio_(k=_odd(o["k"], 2)), ratio_(ra=_odd(o["ratio"], 4)), ratio_(z=_odd(o["z"], 1))]
    ctx.sync()
    assert bad == [E_INVALID] * len(bad), bad
    assert L.ampli_last_error(ctx.h).decode() != ""
    assert reference_(N_=AMPLICON_MAX + 1) == E_RANGE
    msg = L.ampli_last_error(ctx.h).decode()
    assert "AMPLI_AMPLICON_MAX" in msg and str(AMPLICON_MAX) in msg and "N" in msg
    assert ratio_(A_=AMPLICON_MAX + 1) == E_RANGE
    msg = L.ampli_last_error(ctx.h).decode()
    assert "AMPLI_AMPLICON_MAX" in msg and str(AMPLICON_MAX) in msg and "A" in msg
    ctx.sync()
    for v, chk in outs.values():
        chk()
        assert (chk.raw == 0xFF).all()
    # the good calls pass
    assert reference_() == 0 and ratio_(r=o["ref"], st=o["status"]) == 0
    ctx.sync()
    for v, chk in outs.values():
        chk()
    exp = reference(sums, use, 2)
    want = ratios(sums, use, exp)
    assert same(o["ref"].cpu().numpy()[:, 0], exp["med"]) and np.array_equal(o["status"].cpu().numpy(), exp["status"])
    assert same(o["ratio"].cpu().numpy(), want["ratio"]) and same(o["z"].cpu().numpy(), want["z"]) and np.array_equal(o["k"].cpu().numpy(), want["k"])
