"""ampli_exceedance_records refuses bad arguments -- AMPLI_E_INVALID for null pointers, misaligned outputs, P <= 0, negative cut-offs and
first indices and broken records on either side; AMPLI_E_RANGE, with a message that says so, for first_n + n_n > 65534 and P >= 2^31 --
before anything is launched: both outputs, poisoned and fenced, stay untouched."""
import ctypes as C

import numpy as np
import pytest

from amplisolve_amd._lib import Records
from amplisolve_amd.api import EXCEEDANCE_MAX_NORMALS
from tests.exceedance_model import exceedance
from tests.helpers import fenced
from tests.test_gpu_exceedance import ex_records, ref_codes, u16
from tests.test_gpu_parity import _t

pytestmark = pytest.mark.gpu
E_INVALID, E_RANGE = -1, -6
P, NT, NN = 65, 3, 5


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _odd(t, k):
    import torch

    return t.view(torch.uint8).reshape(-1)[k:]


def test_refusals(ctx):
    import torch

    t, n, ref = ex_records(P, NT, 5), ex_records(P, NN, 6), ref_codes(P, 7)
    src_t, src_n = _t(t), _t(n)
    rt, rn = ctx.records(src_t, "i32", NT), ctx.records(src_n, "i32", NN)
    rn16 = ctx.records(ctx.pack(src_n, "u16")[0], "u16", NN)
    d_ref = _t(ref)
    elig, chk_e = fenced((NT, P), torch.int16)
    ge, chk_g = fenced((NT, P, 4, 2), torch.int16)
    L = ctx.lib

    def call(h=ctx.h, t_=rt, n_=rn, P_=P, ref_=d_ref, ncut=100, ccut=100, ft=0, fn=0, skip=0, acc=0, e_=elig, g_=ge):
        return L.ampli_exceedance_records(h, C.byref(t_) if t_ is not None else None, C.byref(n_) if n_ is not None else None, P_, _p(ref_), ncut, ccut, ft, fn,
                                          skip, acc, _p(e_), _p(g_))

    def with_(base, **kw):
        r = Records.from_buffer_copy(base)
        for k, v in kw.items():
            setattr(r, k, v)
        return r

    bad = [call(h=None), call(t_=None), call(n_=None), call(t_=with_(rt, recs=None)), call(n_=with_(rn, recs=None)), call(P_=0), call(P_=-1), call(ncut=-1),
           call(ccut=-1), call(ft=-1), call(fn=-1), call(acc=1, fn=-1),
           call(t_=with_(rt, n_samples=0)), call(n_=with_(rn, n_samples=0)), call(t_=with_(rt, n_samples=-3)), call(n_=with_(rn, n_samples=-3)),
           call(t_=with_(rt, layout=3)), call(n_=with_(rn, layout=-1)), call(t_=with_(rt, E=-1)), call(n_=with_(rn, E=-1)),
           call(ref_=None), call(e_=None), call(g_=None), call(e_=_odd(elig, 1)), call(g_=_odd(ge, 8)), call(g_=_odd(ge, 2)),
           call(t_=with_(rt, row_stride=P - 1)), call(n_=with_(rn, row_stride=P - 1)), call(t_=with_(rt, recs=src_t.data_ptr() + 4)),
           call(n_=with_(rn, recs=src_n.data_ptr() + 4))]
    ctx.sync()
    assert bad == [E_INVALID] * len(bad), bad
    assert L.ampli_last_error(ctx.h).decode() != ""
    assert call(ncut=-1) == E_INVALID and "normal_cutoff" in L.ampli_last_error(ctx.h).decode()
    assert call(n_=with_(rn, recs=src_n.data_ptr() + 4)) == E_INVALID and "normals" in L.ampli_last_error(ctx.h).decode()
    # the ranges: nothing is launched, so the sizes need not be real
    assert call(fn=EXCEEDANCE_MAX_NORMALS - NN + 1) == E_RANGE
    msg = L.ampli_last_error(ctx.h).decode()
    assert "AMPLI_EXCEEDANCE_MAX_NORMALS" in msg and "65534" in msg and "first_n" in msg
    assert call(n_=with_(rn16, n_samples=EXCEEDANCE_MAX_NORMALS + 1)) == E_RANGE and call(fn=1 << 40, acc=1) == E_RANGE
    assert call(P_=(1 << 31) - 1) == E_RANGE and "2^31" in L.ampli_last_error(ctx.h).decode()
    assert call(P_=1 << 40, n_=rn16) == E_RANGE and "2^31" in L.ampli_last_error(ctx.h).decode()
    ctx.sync()
    chk_e(), chk_g()
    assert (chk_e.raw == 0xFF).all() and (chk_g.raw == 0xFF).all()  # nothing written, the payloads included
    assert call(fn=EXCEEDANCE_MAX_NORMALS - NN, ft=1 << 40) == 0     # the last index a panel may have; first_t is free
    ctx.sync()
    chk_e(), chk_g()
    exp = exceedance(t, n, ref)
    assert np.array_equal(u16(elig), exp[0]) and np.array_equal(u16(ge), exp[1])
    assert call(n_=rn16, ncut=0, ccut=0, skip=1, ft=2) == 0         # the other layout, the edges of both cut-offs
    ctx.sync()
    exp = exceedance(t, n, ref, normal_cutoff=0, calling_cutoff=0, first_t=2, skip_same_index=True)
    assert np.array_equal(u16(elig), exp[0]) and np.array_equal(u16(ge), exp[1])
