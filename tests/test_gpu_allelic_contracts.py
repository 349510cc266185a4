"""The output contracts (C25-C27 of include/amplisolve_hip.h) of the three allelic entry points on fenced, poisoned buffers, and their
refusals: AMPLI_E_INVALID / AMPLI_E_RANGE before anything is launched, every output untouched."""
import ctypes as C

import numpy as np
import pytest

from amplisolve_amd._lib import AllelicParams, Records
from tests import allelic_cohorts as ac
from tests import allelic_model as am
from tests.concordance_model import classify, pack_planes
from tests.helpers import fenced
from tests.test_gpu_allelic import _check_sites, _regions
from tests.test_gpu_loo import _pack
from tests.test_gpu_parity import _t

pytestmark = pytest.mark.gpu
E_INVALID, E_RANGE = -1, -6
P, N = 333, 9  # a partial last tile; rows that do not fill a run, a strip or the reference kernel's turns


def _setup(ctx):
    recs = ac.small(P, N, 11, layout_max=65534)
    bits = classify(recs)
    ref = am.reference(recs, bits, P, 100)
    row_g = np.array([0, 0, -1, 3, 4, 99, 6, 7, 8], np.int32)
    exp = am.sites(recs, P, bits, row_g, ref, 100, 2, True)
    return recs, bits, _t(pack_planes(bits, P).view(np.int64)), ref, row_g, exp


@pytest.mark.parametrize("layout", ["i32", "u24", "u16"])
def test_outputs_are_complete_and_in_bounds(ctx, layout):
    import torch

    recs, bits, pl, ref, row_g, exp = _setup(ctx)
    rec = ctx.records(_pack(ctx, recs, layout), layout, N)
    # R adds to every cell of d_ref and writes nothing else: zeros in, the model out, the guards untouched
    r, chk_r = fenced((3, 6, P), torch.int64, poison=0)
    assert ctx.hetsite_reference(rec, P, pl, 100, ref=r).data_ptr() == r.data_ptr()
    ctx.sync()
    chk_r()
    assert np.array_equal(r.cpu().numpy(), ref)
    # S stores every cell of its four planes, untested ones included, whatever they held
    for poison in (0xFF, 0x00):
        bufs = [fenced(sh, dt, poison=poison) for sh, dt in (((N, P), torch.float32), ((N, P, 2), torch.int32), ((N, P), torch.float64), ((N, P), torch.uint8))]
        ctx.allelic_sites(rec, P, pl, _t(row_g), _t(ref), 100, 2, True, *[b[0] for b in bufs])
        ctx.sync()
        for _, chk in bufs:
            chk()
        _check_sites([b[0] for b in bufs], exp)
    # G stores all five sums of every (row, region), empty regions included
    off, pos = _regions(P, 11, 8)
    q, km, v, code = (_t(x) for x in exp[:4])
    want = am.region_sums(*exp[:4], off, pos, 20.0)
    for poison in (0xFF, 0x00):
        s, chk = fenced((N, 11, 5), torch.int64, poison=poison)
        ctx.allelic_regions(q, km, v, code, off, pos, 20.0, out=s)
        ctx.sync()
        chk()
        assert np.array_equal(s.cpu().numpy(), want)


def test_refusals(ctx):
    import torch

    recs, bits, pl, ref, row_g, exp = _setup(ctx)
    src = _t(recs)
    rec = ctx.records(src, "i32", N)
    rec16 = ctx.records(ctx.pack(src, "u16")[0], "u16", N)
    L = ctx.lib
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    odd = lambda t, k: t.view(torch.uint8).reshape(-1)[k:]
    err = lambda: L.ampli_last_error(ctx.h).decode()

    def with_(base=rec, **kw):
        r = Records.from_buffer_copy(base)
        for k, v in kw.items():
            setattr(r, k, v)
        return r

    # ---- R ----
    dref, chk_ref = fenced((3, 6, P), torch.int64)

    def call_r(h=ctx.h, r=rec, P_=P, a=pl, md=100, o=dref):
        return L.ampli_hetsite_reference_records(h, C.byref(r) if r is not None else None, P_, p(a), md, p(o))

    bad = [call_r(h=None), call_r(r=None), call_r(r=with_(recs=None)), call_r(P_=0), call_r(P_=-1), call_r(r=with_(n_samples=0)), call_r(r=with_(layout=3)),
           call_r(r=with_(E=-1)), call_r(a=None), call_r(o=None), call_r(md=0), call_r(md=-5), call_r(a=odd(pl, 4)), call_r(o=odd(dref, 4)),
           call_r(r=with_(row_stride=P - 1))]
    assert bad == [E_INVALID] * len(bad), bad
    assert err() != ""
    assert call_r(P_=(1 << 31) - 1) == E_RANGE and "2^31" in err()
    assert call_r(P_=1 << 40, r=rec16) == E_RANGE and "2^31" in err()
    assert call_r(P_=1 << 28) == E_RANGE and "2^28" in err() and "int32" in err()
    ctx.sync()
    chk_ref()
    assert (chk_ref.raw == 0xFF).all()

    # ---- S ----
    dr, drow = _t(ref), _t(row_g)
    outs = [fenced(sh, dt) for sh, dt in (((N, P), torch.float32), ((N, P, 2), torch.int32), ((N, P), torch.float64), ((N, P), torch.uint8))]
    oq, okm, ov, oc = (o[0] for o in outs)
    good = AllelicParams(100, 2, 1)

    def call_s(h=ctx.h, r=rec, P_=P, a=pl, n_g=N, g=drow, f=dr, prm=good, q=oq, km=okm, v=ov, c=oc):
        return L.ampli_allelic_site_records(h, C.byref(r) if r is not None else None, P_, p(a), n_g, p(g), p(f), C.byref(prm) if prm is not None else None,
                                            p(q), p(km), p(v), p(c))

    bad = [call_s(h=None), call_s(r=None), call_s(P_=0), call_s(r=with_(n_samples=-3)), call_s(r=with_(layout=-1)), call_s(a=None), call_s(n_g=0), call_s(n_g=-1),
           call_s(g=None), call_s(f=None), call_s(prm=None), call_s(q=None), call_s(km=None), call_s(v=None), call_s(c=None), call_s(a=odd(pl, 4)),
           call_s(g=odd(drow, 2)), call_s(f=odd(dr, 4)), call_s(q=odd(oq, 2)), call_s(km=odd(okm, 4)), call_s(v=odd(ov, 4)),
           call_s(prm=AllelicParams(0, 2, 1)), call_s(prm=AllelicParams(100, 0, 1)), call_s(prm=AllelicParams(100, 2, 2)), call_s(prm=AllelicParams(100, 2, -1)),
           call_s(r=with_(recs=src.data_ptr() + 4))]
    assert bad == [E_INVALID] * len(bad), bad
    assert call_s(P_=1 << 31) == E_RANGE and "2^31" in err()
    assert call_s(r=with_(n_samples=4194241), P_=1) == E_RANGE and "n_samples" in err()
    ctx.sync()
    for o, chk in outs:
        chk()
        assert (chk.raw == 0xFF).all()

    # ---- G ----
    q, km, v, code = (_t(x) for x in exp[:4])
    off = _t(np.array([0, 10, 10, 40], np.int32))
    pos = _t(np.arange(40, dtype=np.int32))
    ds, chk_s = fenced((N, 3, 5), torch.int64)

    def call_g(h=ctx.h, q_=q, km_=km, v_=v, c_=code, S=N, P_=P, R=3, o_=off, p_=pos, W=40, sq=20.0, s_=ds):
        return L.ampli_allelic_region_sums(h, p(q_), p(km_), p(v_), p(c_), S, P_, R, p(o_), p(p_), W, sq, p(s_))

    bad = [call_g(h=None), call_g(q_=None), call_g(km_=None), call_g(v_=None), call_g(c_=None), call_g(o_=None), call_g(p_=None), call_g(s_=None), call_g(S=0),
           call_g(P_=0), call_g(R=0), call_g(W=-1), call_g(sq=-1.0), call_g(sq=float("nan")), call_g(q_=odd(q, 2)), call_g(km_=odd(km, 4)), call_g(v_=odd(v, 4)),
           call_g(o_=odd(off, 2)), call_g(p_=odd(pos, 2)), call_g(s_=odd(ds, 4))]
    assert bad == [E_INVALID] * len(bad), bad
    assert call_g(W=1 << 27) == E_RANGE and "2^27" in err()
    assert call_g(P_=1 << 31) == E_RANGE and "2^31" in err()
    assert call_g(S=2097121) == E_RANGE and "2097120" in err()
    ctx.sync()
    chk_s()
    assert (chk_s.raw == 0xFF).all()

    # the good calls pass
    assert call_s() == 0 and call_g() == 0
    dref.zero_()
    assert call_r() == 0 and call_r(r=rec16) == 0
    ctx.sync()
    for _, chk in outs + [(None, chk_ref), (None, chk_s)]:
        chk()
    assert np.array_equal(dref.cpu().numpy(), 2 * ref)
    _check_sites((oq, okm, ov, oc), exp)
    assert np.array_equal(ds.cpu().numpy(), am.region_sums(*exp[:4], np.array([0, 10, 10, 40]), np.arange(40), 20.0))
