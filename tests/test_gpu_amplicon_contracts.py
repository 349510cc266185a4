"""The output contracts C13-C15 of the amplicon entry points (include/amplisolve_hip.h) on poisoned, fenced buffers (tests/helpers.py):
every cell of the chunk's rows written whatever the matrix held -- empty lists included, with plain stores: the other chunks' rows keep
what they held -- and nothing written outside.  What is read ends where its buffer ends: a list whose last entry is P - 1 of a record
buffer that ends there, amp_off of exactly A + 1 and amp_pos of exactly W words, sums, use, reference and status of exactly their
sizes."""
import ctypes as C

import numpy as np
import pytest

from tests.amplicon_model import depth_sums, ratios, reference, same
from tests.concordance_cohorts import records
from tests.helpers import fenced
from tests.test_gpu_amplicon import lists, matrix
from tests.test_gpu_loo import _pack

pytestmark = pytest.mark.gpu


def _fenced_copy(t):
    buf, chk = fenced(tuple(t.shape), t.dtype)
    buf.copy_(t)
    return buf, chk


@pytest.mark.parametrize("layout", ["i32", "u24", "u16"])
@pytest.mark.parametrize("P", [65, 1000])
def test_depth_sums_of_a_chunk(ctx, layout, P):
    import torch

    n, lo, hi = 19, 9, 19  # the chunk: ten rows, a strip of eight and one of two
    recs = records(P, n, P + n)
    off, pos = lists(P)    # the last list's last entry is P - 1, the last entry of amp_pos
    assert pos[-1] == P - 1 and off[-1] == len(pos)
    exp = depth_sums(recs, off, pos)
    A = len(off) - 1
    src, chk_src = _fenced_copy(_pack(ctx, recs[lo:hi], layout))  # the records end where their buffer ends
    d_off, chk_off = _fenced_copy(torch.from_numpy(off.astype(np.int32)))
    d_pos, chk_pos = _fenced_copy(torch.from_numpy(pos.astype(np.int32)))
    buf, chk = fenced((n, A, 4), torch.int64)
    before = src.clone()
    ctx.amplicon_depth(ctx.records(src, layout, hi - lo), P, d_off, d_pos, out=buf[lo:hi])
    ctx.sync()
    chk(), chk_src(), chk_off(), chk_pos()
    got = buf.cpu().numpy()
    assert (got[:lo] == -1).all()                   # the earlier chunk's rows: not this call's
    assert np.array_equal(got[lo:hi], exp[lo:hi])   # every sum of the chunk's rows, the empty lists' zeros included: no poison left
    assert torch.equal(src, before) and np.array_equal(d_off.cpu().numpy(), off.astype(np.int32)) and np.array_equal(d_pos.cpu().numpy(), pos.astype(np.int32))
    ctx.amplicon_depth(ctx.records(_pack(ctx, recs[:lo], layout), layout, lo), P, d_off, d_pos, out=buf[:lo])
    ctx.amplicon_depth(ctx.records(src, layout, hi - lo), P, d_off, d_pos, out=buf[lo:hi])  # again, over its own results
    ctx.sync()
    chk()
    assert np.array_equal(buf.cpu().numpy(), exp)


def test_the_sums_end_where_their_buffer_ends(ctx):
    """the last row's last amplicon is the last 32 bytes of the payload; with empty lists only, every cell is still written"""
    import torch

    P, n = 65, 8
    recs = records(P, n, 5)
    off = np.zeros(4, np.int32)
    d_pos, chk_pos = fenced((1,), torch.int32)
    buf, chk = fenced((n, 3, 4), torch.int64)
    rec, d_off = ctx.records(_pack(ctx, recs, "u16"), "u16", n), torch.from_numpy(off).cuda()
    # W = 0: amp_pos is a valid pointer that is never read through
    assert ctx.lib.ampli_amplicon_depth_records(ctx.h, C.byref(rec), P, 3, d_off.data_ptr(), d_pos.data_ptr(), 0, 100, buf.data_ptr()) == 0
    ctx.sync()
    chk(), chk_pos()
    assert (buf.cpu().numpy() == 0).all()


@pytest.mark.parametrize("N,A", [(3, 2), (65, 65), (257, 1000)])
def test_reference_and_ratios(ctx, N, A):
    import torch

    sums, use = matrix(N, A)
    exp = reference(sums, use, 2)
    d_sums, chk_sums = _fenced_copy(torch.from_numpy(np.ascontiguousarray(sums)))
    d_use, chk_use = _fenced_copy(torch.from_numpy(np.ascontiguousarray(use)))
    total, chk_total = fenced((N,), torch.int64)
    ref, chk_ref = fenced((A, 2), torch.float64)
    status, chk_status = fenced((A,), torch.uint8)
    p = lambda t: t.data_ptr()
    L = ctx.lib
    assert L.ampli_amplicon_reference(ctx.h, p(d_sums), N, A, p(d_use), 2, p(total), p(ref), p(status)) == 0
    ctx.sync()
    for c in (chk_sums, chk_use, chk_total, chk_ref, chk_status):
        c()
    assert np.array_equal(total.cpu().numpy(), exp["total"]) and np.array_equal(status.cpu().numpy(), exp["status"])  # no poison left
    got = ref.cpu().numpy()
    assert same(got[:, 0], exp["med"]) and same(got[:, 1], exp["mad"])
    nan = np.isnan(got)
    assert (got[nan].view(np.uint64) == 0x7FF8000000000000).all()  # not the poison's NaN
    assert np.array_equal(d_sums.cpu().numpy(), sums) and np.array_equal(d_use.cpu().numpy(), use)

    want = ratios(sums, use, exp)
    total.fill_(-1)
    centre, chk_centre = fenced((N,), torch.float64)
    k, chk_k = fenced((N,), torch.int32)
    ratio, chk_ratio = fenced((N, A), torch.float64)
    z, chk_z = fenced((N, A), torch.float64)
    ref0, status0 = ref.clone(), status.clone()
    assert L.ampli_amplicon_ratio(ctx.h, p(d_sums), N, A, p(d_use), p(ref), p(status), p(total), p(centre), p(k), p(ratio), p(z)) == 0
    ctx.sync()
    for c in (chk_sums, chk_use, chk_total, chk_ref, chk_status, chk_centre, chk_k, chk_ratio, chk_z):
        c()
    assert np.array_equal(total.cpu().numpy(), want["total"]) and np.array_equal(k.cpu().numpy(), want["k"])
    assert same(centre.cpu().numpy(), want["centre"]) and same(ratio.cpu().numpy(), want["ratio"]) and same(z.cpu().numpy(), want["z"])
    for t in (centre, ratio, z):
        v = t.cpu().numpy()
        assert (v[np.isnan(v)].view(np.uint64) == 0x7FF8000000000000).all()
    assert torch.equal(ref.view(torch.int64), ref0.view(torch.int64)) and torch.equal(status, status0)
    assert np.array_equal(d_sums.cpu().numpy(), sums) and np.array_equal(d_use.cpu().numpy(), use)
