"""ampli_genotype_planes_records and ampli_concordance_pairs refuse bad arguments with AMPLI_E_INVALID before anything is launched:
the outputs, poisoned and fenced, stay untouched."""
import ctypes as C

import numpy as np
import pytest

from amplisolve_amd._lib import GenotypeParams, Records
from tests.concordance_cohorts import records
from tests.concordance_model import DEFAULTS, planes, words
from tests.helpers import fenced
from tests.test_gpu_parity import _t

pytestmark = pytest.mark.gpu
E_INVALID = -1
P, N = 130, 4


def _params(**kw):
    return GenotypeParams(*[dict(DEFAULTS, **kw)[k] for k in DEFAULTS])


def test_planes_refusals(ctx):
    import torch

    recs = records(P, N, 5)
    src = _t(recs)
    rec = ctx.records(src, "i32", N)
    out, chk = fenced((N, 6, words(P)), torch.int64)
    L = ctx.lib
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None

    def call(h=ctx.h, r=rec, P_=P, prm=_params(), o=out):
        return L.ampli_genotype_planes_records(h, C.byref(r) if r is not None else None, P_, C.byref(prm) if prm is not None else None, p(o))

    def with_(**kw):
        r = Records.from_buffer_copy(rec)
        for k, v in kw.items():
            setattr(r, k, v)
        return r

    bad = [call(h=None), call(r=None), call(r=with_(recs=None)), call(P_=0), call(P_=-1), call(r=with_(n_samples=0)), call(r=with_(n_samples=-3)),
           call(r=with_(layout=3)), call(r=with_(layout=-1)), call(r=with_(E=-1)), call(prm=None), call(o=None), call(o=out.view(torch.uint8).reshape(-1)[4:]),
           call(r=with_(row_stride=P - 1)), call(r=with_(recs=src.data_ptr() + 4))]
    violated = [dict(min_depth=0), dict(min_depth=-1), dict(absent_max_pm=-1), dict(absent_max_pm=250), dict(het_min_pm=100), dict(het_min_pm=751),
                dict(het_max_pm=249), dict(het_max_pm=900), dict(hom_min_pm=750), dict(hom_min_pm=1001)]
    bad += [call(prm=_params(**kw)) for kw in violated]
    ctx.sync()
    assert bad == [E_INVALID] * len(bad), bad
    assert L.ampli_last_error(ctx.h).decode() != ""
    chk()
    assert (chk.raw == 0xFF).all()  # nothing written, the payload included
    assert call() == 0 and call(prm=_params(het_min_pm=750)) == 0 and call(prm=_params(absent_max_pm=0, hom_min_pm=1000)) == 0  # the good calls pass
    ctx.sync()
    assert np.array_equal(out.cpu().numpy().view(np.uint64), planes(recs, P, absent_max_pm=0, hom_min_pm=1000))


def test_pairs_refusals(ctx):
    import torch

    pl = _t(planes(records(P, N, 5), P).view(np.int64))
    counts, chk = fenced((N, N, 5), torch.int32)
    L = ctx.lib
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None

    def call(h=ctx.h, P_=P, a=pl, n_a=N, b=pl, n_b=N, o=counts):
        return L.ampli_concordance_pairs(h, P_, p(a), n_a, p(b), n_b, p(o))

    bad = [call(h=None), call(P_=0), call(P_=-64), call(a=None), call(b=None), call(o=None), call(n_a=0), call(n_b=0), call(n_a=-1), call(n_b=-2),
           call(a=pl.view(torch.uint8).reshape(-1)[4:]), call(b=pl.view(torch.uint8).reshape(-1)[4:]), call(o=counts.view(torch.uint8).reshape(-1)[2:])]
    ctx.sync()
    assert bad == [E_INVALID] * len(bad), bad
    chk()
    assert (chk.raw == 0xFF).all()
    assert call() == 0
    ctx.sync()
    chk()
    assert (counts.cpu().numpy() >= 0).all()
