"""ampli_contamination_records refuses bad arguments -- AMPLI_E_INVALID for null or misaligned pointers, n_b <= 0, P <= 0 and broken
records; AMPLI_E_RANGE, with a message that says so, for P >= 2^31 and for P >= 2^28 with int32 records -- before anything is launched
or cleared: the output, poisoned and fenced, stays untouched."""
import ctypes as C

import numpy as np
import pytest

from amplisolve_amd._lib import Records
from tests.concordance_cohorts import records
from tests.concordance_model import classify, pack_planes
from tests.contamination_model import sums
from tests.helpers import fenced
from tests.test_gpu_parity import _t

pytestmark = pytest.mark.gpu
E_INVALID, E_RANGE = -1, -6
P, N, NB = 1000, 4, 5  # 16 words and 4 waves: a good call clears the matrix and adds four slices into it


def test_refusals(ctx):
    import torch

    recs = records(P, N, 5)
    bits = classify(recs)
    bits_b = classify(records(P, NB, 6))
    src = _t(recs)
    rec = ctx.records(src, "i32", N)
    rec16 = ctx.records(ctx.pack(src, "u16")[0], "u16", N)
    pa, pb = _t(pack_planes(bits, P).view(np.int64)), _t(pack_planes(bits_b, P).view(np.int64))
    out, chk = fenced((N, NB, 9), torch.int64)
    L = ctx.lib
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    odd = lambda t, k: t.view(torch.uint8).reshape(-1)[k:]

    def call(h=ctx.h, r=rec, P_=P, a=pa, b=pb, n_b=NB, o=out):
        return L.ampli_contamination_records(h, C.byref(r) if r is not None else None, P_, p(a), p(b), n_b, p(o))

    def with_(base=rec, **kw):
        r = Records.from_buffer_copy(base)
        for k, v in kw.items():
            setattr(r, k, v)
        return r

    bad = [call(h=None), call(r=None), call(r=with_(recs=None)), call(P_=0), call(P_=-1), call(r=with_(n_samples=0)), call(r=with_(n_samples=-3)),
           call(r=with_(layout=3)), call(r=with_(layout=-1)), call(r=with_(E=-1)), call(a=None), call(b=None), call(o=None), call(n_b=0), call(n_b=-2),
           call(a=odd(pa, 4)), call(b=odd(pb, 4)), call(o=odd(out, 4)), call(o=odd(out, 1)), call(r=with_(row_stride=P - 1)),
           call(r=with_(recs=src.data_ptr() + 4))]
    ctx.sync()
    assert bad == [E_INVALID] * len(bad), bad
    assert L.ampli_last_error(ctx.h).decode() != ""
    # the ranges: nothing is launched, so the sizes need not be real
    assert call(P_=(1 << 31) - 1) == E_RANGE and "2^31" in L.ampli_last_error(ctx.h).decode()
    assert call(P_=1 << 31) == E_RANGE and call(P_=1 << 40, r=rec16) == E_RANGE and "2^31" in L.ampli_last_error(ctx.h).decode()
    assert call(P_=1 << 28) == E_RANGE
    msg = L.ampli_last_error(ctx.h).decode()
    assert "2^28" in msg and "int32" in msg
    assert call(P_=(1 << 30) + 5) == E_RANGE and "2^28" in L.ampli_last_error(ctx.h).decode()
    assert call(n_b=4194241) == E_RANGE and "n_b" in L.ampli_last_error(ctx.h).decode()
    ctx.sync()
    chk()
    assert (chk.raw == 0xFF).all()  # nothing written or cleared, the payload included
    assert call() == 0 and call(r=rec16) == 0  # the good calls pass
    ctx.sync()
    chk()
    assert np.array_equal(out.cpu().numpy(), sums(recs, bits, bits_b))
