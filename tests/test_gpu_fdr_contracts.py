"""The output contract C20 (include/amplisolve_hip.h) of ampli_fdr_adjust on poisoned, fenced buffers (tests/helpers.py): d_a, d_m and
d_rank are fully overwritten and nothing beyond them is, the workspace is written only inside ampli_fdr_workspace_bytes, d_s is never
written, and every refusal comes with its code and leaves the outputs untouched."""
import ctypes as C

import numpy as np
import pytest

from tests import fdr_model as fm
from tests import fdr_planes as fp
from tests.helpers import fenced

pytestmark = pytest.mark.gpu
E_INVALID, E_RANGE = -1, -6


def _fenced_copy(t):
    import torch

    buf, chk = fenced(tuple(t.shape), torch.float32)
    buf.copy_(torch.from_numpy(np.array(t)))  # a copy: the shared case is read-only
    return buf, chk


def _buffers(ctx, rows, P):
    import torch

    a, chk_a = fenced((rows, P, 4), torch.float32)
    m, chk_m = fenced((rows,), torch.int32)
    r, chk_r = fenced((rows, P, 4), torch.int32)
    work, chk_w = fenced((ctx.fdr_workspace_bytes(rows, P),), torch.uint8)  # exactly the query's bytes
    return (a, m, r, work), (chk_a, chk_m, chk_r, chk_w)


@pytest.mark.parametrize("two_sided", [False, True])
@pytest.mark.parametrize("P,lo,hi", [(1, 0, 1), (65, 1, 4), (fp.TILE_KEYS // 4 + 1, 4, 9), (2 * (fp.TILE_KEYS // 4) - 1, 9, 12)])
def test_outputs_are_fully_overwritten_and_nothing_else_is_written(ctx, P, lo, hi, two_sided):
    import torch

    s, A, m, R = fp.case(P, two_sided)
    rows = hi - lo
    d_s, chk_s = _fenced_copy(s[lo:hi])
    (a, mm, r, work), checks = _buffers(ctx, rows, P)
    before = d_s.clone()
    for with_rank in (True, False, True):
        for c in checks:
            c.repoison()
        ctx.fdr_adjust(d_s, two_sided, a=a, m=mm, rank=r if with_rank else False, work=work)
        ctx.sync()
        [c() for c in checks + (chk_s,)]
        got_a, got_m, got_r = a.cpu().numpy(), mm.cpu().numpy(), r.cpu().numpy()
        assert not np.isnan(got_a).any() and (got_m >= 0).all()  # over the poison: every cell written
        if with_rank:
            assert (got_r >= 0).all()
            fm.compare(got_a, got_m, got_r, A[lo:hi], m[lo:hi], R[lo:hi])
        else:
            assert (checks[2].raw == 0xFF).all()  # d_rank NULL: the buffer is not a hidden argument
            fm.compare(got_a, got_m, None, A[lo:hi], m[lo:hi], R[lo:hi])
        assert d_s.view(torch.int32).equal(before.view(torch.int32))  # the plane is byte-identical afterwards (it holds NaNs)
        assert d_s.cpu().numpy().tobytes() == s[lo:hi].tobytes()


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _odd(t, k):
    import torch

    return t.view(torch.uint8).reshape(-1)[k:]


def test_refusals(ctx):
    P, rows = 65, 3
    s, A, m, R = fp.case(P, False)
    d_s, chk_s = _fenced_copy(s[:rows])
    (a, mm, r, work), checks = _buffers(ctx, rows, P)
    L = ctx.lib
    need = ctx.fdr_workspace_bytes(rows, P)

    def adjust(h=ctx.h, s_=d_s, rows_=rows, P_=P, two=0, w=work, wb=need, a_=a, m_=mm, r_=r):
        return L.ampli_fdr_adjust(h, _p(s_), rows_, P_, two, _p(w), wb, _p(a_), _p(m_), _p(r_))

    bad = [adjust(h=None), adjust(s_=None), adjust(a_=None), adjust(m_=None), adjust(w=None), adjust(rows_=0), adjust(rows_=-2), adjust(P_=0), adjust(P_=-1),
           adjust(two=2), adjust(two=-1), adjust(s_=_odd(d_s, 4)), adjust(s_=_odd(d_s, 8)), adjust(a_=_odd(a, 4)), adjust(a_=_odd(a, 8)), adjust(m_=_odd(mm, 2)),
           adjust(r_=_odd(r, 4)), adjust(w=_odd(work, 4)), adjust(wb=need - 1), adjust(wb=0), adjust(rows_=rows + 1), adjust(P_=P + 1)]  # the last two: a workspace too small
    ctx.sync()
    assert bad == [E_INVALID] * len(bad), bad
    assert adjust(wb=need - 1) == E_INVALID and "workspace" in L.ampli_last_error(ctx.h).decode()
    # the range: nothing is launched, so the sizes need not be real
    for rc in (adjust(P_=1 << 29), adjust(P_=1 << 40), adjust(P_=(1 << 29) + 5, wb=1 << 62)):
        assert rc == E_RANGE and "2^31" in L.ampli_last_error(ctx.h).decode()
    ctx.sync()
    for c in checks + (chk_s,):
        c()
    for c in checks:
        assert (c.raw == 0xFF).all()  # nothing written, the payloads included
    assert adjust() == 0 and adjust(r_=None) == 0 and adjust() == 0
    ctx.sync()
    [c() for c in checks + (chk_s,)]
    fm.compare(a.cpu().numpy(), mm.cpu().numpy(), r.cpu().numpy(), A[:rows], m[:rows], R[:rows])
