"""The output contract C17 of ampli_exceedance_records (include/amplisolve_hip.h) on poisoned, fenced buffers (tests/helpers.py): with
accumulate == 0 every cell of d_elig and d_ge is written whatever they held, the NA cells included, and nothing outside; with accumulate
!= 0 the counts are added onto what the first chunk left, NA stays NA, and nothing is written outside either.  What is read ends where its
buffer ends: the tumours' records, the normals' records and the reference codes."""
import numpy as np
import pytest

from tests.exceedance_model import NA, exceedance
from tests.helpers import fenced
from tests.test_gpu_exceedance import ROWS, STRIP, ex_records, ref_codes, u16
from tests.test_gpu_loo import _pack

pytestmark = pytest.mark.gpu


def _fenced_copy(t):
    buf, chk = fenced(tuple(t.shape), t.dtype)
    buf.copy_(t)
    return buf, chk


@pytest.mark.parametrize("lt,ln", [("i32", "u16"), ("u24", "u24"), ("u16", "i32")])
@pytest.mark.parametrize("P", [1, 65, 1000])
def test_overwrite_then_accumulate(ctx, lt, ln, P):
    import torch

    n_t, n_n, cut = ROWS + 3, 2 * STRIP + 3, STRIP + 1   # a row group and a partial one; the normals in two chunks, a strip and one row first
    t, n, ref = ex_records(P, n_t, P + 1), ex_records(P, n_n, P + 2), ref_codes(P, P)
    src_t, chk_t = _fenced_copy(_pack(ctx, t, lt))        # the records end where their buffers end
    src_a, chk_a = _fenced_copy(_pack(ctx, n[:cut], ln))
    src_b, chk_b = _fenced_copy(_pack(ctx, n[cut:], ln))
    d_ref, chk_ref = _fenced_copy(torch.from_numpy(ref.copy()))
    elig, chk_e = fenced((n_t, P), torch.int16)
    ge, chk_g = fenced((n_t, P, 4, 2), torch.int16)
    before = [x.clone() for x in (src_t, src_a, src_b)]
    rt = ctx.records(src_t, lt, n_t)
    ctx.exceedance(rt, ctx.records(src_a, ln, cut), P, d_ref, first_t=50, first_n=0, elig=elig, ge=ge)
    ctx.sync()
    for chk in (chk_e, chk_g, chk_t, chk_a, chk_b, chk_ref):
        chk()
    e1, g1 = exceedance(t, n[:cut], ref, first_t=50)
    assert np.array_equal(u16(elig), e1) and np.array_equal(u16(ge), g1)  # every cell over the poison: 0xFFFF is NA only where NA is due
    ctx.exceedance(rt, ctx.records(src_b, ln, n_n - cut), P, d_ref, first_t=50, first_n=cut, accumulate=True, elig=elig, ge=ge)
    ctx.sync()
    for chk in (chk_e, chk_g, chk_t, chk_a, chk_b, chk_ref):
        chk()
    e2, g2 = exceedance(t, n, ref, first_t=50)
    assert np.array_equal(u16(elig), e2) and np.array_equal(u16(ge), g2) and np.array_equal(g1 == NA, g2 == NA)
    assert all(torch.equal(a, b) for a, b in zip((src_t, src_a, src_b), before)) and np.array_equal(d_ref.cpu().numpy(), ref)
    ctx.exceedance(rt, ctx.records(src_a, ln, cut), P, d_ref, first_t=50, first_n=0, elig=elig, ge=ge)  # again, over its own results
    ctx.sync()
    chk_e(), chk_g()
    assert np.array_equal(u16(elig), e1) and np.array_equal(u16(ge), g1)


def test_rows_of_a_larger_matrix(ctx):
    """a chunk of tumours writes its rows of the outputs and leaves the other chunks' rows as they are"""
    import torch

    P, n_t, lo, n_n = 130, ROWS + 5, ROWS - 1, 5
    t, n, ref = ex_records(P, n_t, 5), ex_records(P, n_n, 6), ref_codes(P, 7)
    elig, chk_e = fenced((n_t, P), torch.int16)
    ge, chk_g = fenced((n_t, P, 4, 2), torch.int16)
    rn = ctx.records(_pack(ctx, n, "u16"), "u16", n_n)
    ctx.exceedance(ctx.records(_pack(ctx, t[lo:], "u16"), "u16", n_t - lo), rn, P, ref, first_t=lo, first_n=3, skip_same_index=True, elig=elig[lo:], ge=ge[lo:])
    ctx.sync()
    chk_e(), chk_g()
    exp = exceedance(t, n, ref, first_n=3, skip_same_index=True)
    assert (u16(elig)[:lo] == 0xFFFF).all() and (u16(ge)[:lo] == 0xFFFF).all()
    assert np.array_equal(u16(elig)[lo:], exp[0][lo:]) and np.array_equal(u16(ge)[lo:], exp[1][lo:])
    ctx.exceedance(ctx.records(_pack(ctx, t[:lo], "u16"), "u16", lo), rn, P, ref, first_t=0, first_n=3, skip_same_index=True, elig=elig[:lo], ge=ge[:lo])
    ctx.sync()
    chk_e(), chk_g()
    assert np.array_equal(u16(elig), exp[0]) and np.array_equal(u16(ge), exp[1]) and (exp[0] < n_n).any()
