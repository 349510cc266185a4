"""ampli_spectrum_records refuses bad arguments -- AMPLI_E_INVALID for null pointers, a misaligned d_sums, P <= 0, C <= 0, a negative
cut-off, max_alt_pm outside [0, 1000] and broken records; AMPLI_E_RANGE, with a message that says so, for C > 128 and P >= 2^31 --
before anything is launched or cleared: the output, poisoned and fenced, stays untouched."""
import ctypes as C

import numpy as np
import pytest

from amplisolve_amd._lib import Records
from amplisolve_amd.api import SPECTRUM_MAX_CLASSES
from tests.helpers import fenced
from tests.spectrum_model import class_sums
from tests.test_gpu_parity import _t
from tests.test_gpu_spectrum import classes, spec_records

pytestmark = pytest.mark.gpu
E_INVALID, E_RANGE = -1, -6
P, N, NC = 65, 5, 68


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _odd(t, k):
    import torch

    return t.view(torch.uint8).reshape(-1)[k:]


def test_refusals(ctx):
    import torch

    recs, ref = spec_records(P, N, 5)
    cls = classes(P, NC, 6)
    src = _t(recs)
    rec = ctx.records(src, "i32", N)
    rec16 = ctx.records(ctx.pack(src, "u16")[0], "u16", N)
    d_ref, d_cls = _t(ref), _t(cls)
    out, chk = fenced((N, NC, 9), torch.int64)
    L = ctx.lib

    def call(h=ctx.h, r=rec, P_=P, ref_=d_ref, cls_=d_cls, C_=NC, cov=100, pm=30, out_=out):
        return L.ampli_spectrum_records(h, C.byref(r) if r is not None else None, P_, _p(ref_), _p(cls_), C_, cov, pm, _p(out_))

    def with_(base=rec, **kw):
        r = Records.from_buffer_copy(base)
        for k, v in kw.items():
            setattr(r, k, v)
        return r

    assert L.ampli_last_spectrum_segments(None) == E_INVALID
    bad = [call(h=None), call(r=None), call(r=with_(recs=None)), call(P_=0), call(P_=-1), call(C_=0), call(C_=-2), call(cov=-1), call(pm=-1), call(pm=1001),
           call(r=with_(n_samples=0)), call(r=with_(n_samples=-3)), call(r=with_(layout=3)), call(r=with_(layout=-1)), call(r=with_(E=-1)),
           call(ref_=None), call(cls_=None), call(out_=None), call(out_=_odd(out, 4)), call(out_=_odd(out, 1)),
           call(r=with_(row_stride=P - 1)), call(r=with_(recs=src.data_ptr() + 4))]
    ctx.sync()
    assert bad == [E_INVALID] * len(bad), bad
    assert L.ampli_last_error(ctx.h).decode() != ""
    assert call(pm=1001) == E_INVALID and "max_alt_pm" in L.ampli_last_error(ctx.h).decode()
    # the ranges: nothing is launched, so the sizes need not be real
    assert call(C_=SPECTRUM_MAX_CLASSES + 1) == E_RANGE
    msg = L.ampli_last_error(ctx.h).decode()
    assert "AMPLI_SPECTRUM_MAX_CLASSES" in msg and "128" in msg and "C" in msg
    assert call(C_=1 << 30, r=rec16) == E_RANGE
    assert call(P_=(1 << 31) - 1) == E_RANGE and "2^31" in L.ampli_last_error(ctx.h).decode()
    assert call(P_=1 << 40, r=rec16) == E_RANGE and "2^31" in L.ampli_last_error(ctx.h).decode()
    ctx.sync()
    chk()
    assert (chk.raw == 0xFF).all()  # nothing written, the payload included
    assert call() == 0 and L.ampli_last_spectrum_segments(ctx.h) == 1
    ctx.sync()
    chk()
    assert np.array_equal(out.cpu().numpy(), class_sums(recs, ref, cls, NC))
    assert call(r=rec16, cov=0, pm=1000) == 0 and call(r=rec16, cov=0, pm=0) == 0  # the other layout, the edges of both parameters
    ctx.sync()
    assert np.array_equal(out.cpu().numpy(), class_sums(recs, ref, cls, NC, 0, 0))
