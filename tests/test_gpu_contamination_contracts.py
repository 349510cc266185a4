"""The output contract of ampli_contamination_records (include/amplisolve_hip.h, C12) on poisoned, fenced buffers (tests/helpers.py):
every one of the chunk's [n][n_b][9] sums overwritten whatever the matrix held -- with one position slice (plain stores) and with several
(the call clears its rows, the slices add into them) -- nothing outside written, the other chunks' rows of the same matrix included, and
the records and both plane sets unchanged.  Plane rows beyond n / n_b and plane words beyond W are never read: the plane sets end where
their fenced buffers end, and sources past n_b hold a pattern that would change every sum."""
import numpy as np
import pytest

from tests.concordance_cohorts import records
from tests.concordance_model import classify, pack_planes
from tests.contamination_model import sums
from tests.helpers import fenced
from tests.test_gpu_loo import _pack

pytestmark = pytest.mark.gpu


# slices (256 compute units): (77, 7, 65) one; (1000, 7, 130) 16 words, 21 waves -> four of 4 words; (4200, 7, 70) 14, the last of 1 word
@pytest.mark.parametrize("layout", ["i32", "u24", "u16"])
@pytest.mark.parametrize("P,n_b", [(77, 65), (1000, 130), (4200, 70), (64, 1)])
def test_sums_of_a_chunk(ctx, layout, P, n_b):
    import torch

    n, lo, hi = 7, 3, 7
    recs = records(P, n, P + n)
    bits_a = classify(recs)
    bits_b = classify(records(P, 130, 1000 + P))[:n_b + 2]
    exp = sums(recs, bits_a, bits_b[:n_b])
    pa = torch.from_numpy(pack_planes(bits_a, P).view(np.int64)).cuda()
    pb = torch.from_numpy(pack_planes(bits_b, P).view(np.int64)).cuda()  # two rows more than n_b: never read
    buf, chk = fenced((n, n_b, 9), torch.int64)
    src = _pack(ctx, recs[lo:hi], layout)
    before, pa0, pb0 = src.clone(), pa.clone(), pb.clone()
    ctx.contamination(ctx.records(src, layout, hi - lo), P, pa[lo:hi], pb[:n_b], out=buf[lo:hi])
    ctx.sync()
    chk()
    got = buf.cpu().numpy()
    assert (got[:lo] == -1).all()                   # the earlier chunk's rows: not this call's
    assert np.array_equal(got[lo:hi], exp[lo:hi])   # every sum of the chunk's rows: no poison left, none added to
    assert torch.equal(src, before) and torch.equal(pa, pa0) and torch.equal(pb, pb0)
    ctx.contamination(ctx.records(_pack(ctx, recs[:lo], layout), layout, lo), P, pa[:lo], pb[:n_b], out=buf[:lo])
    ctx.contamination(ctx.records(src, layout, hi - lo), P, pa[lo:hi], pb[:n_b], out=buf[lo:hi])  # again, over its own results
    ctx.sync()
    chk()
    assert np.array_equal(buf.cpu().numpy(), exp)


def test_planes_end_where_their_buffers_end(ctx):
    """both plane sets in fenced buffers of exactly [n][6][W] and [n_b][6][W] words: a read past either would fault or go unnoticed,
    a write would not -- the guards hold"""
    import torch

    P, n, n_b = 1000, 5, 65
    recs = records(P, n, P + n)
    bits_a, bits_b = classify(recs), classify(records(P, 130, 1000 + P))[:n_b]
    pa, chk_a = fenced((n, 6, 16), torch.int64)
    pb, chk_b = fenced((n_b, 6, 16), torch.int64)
    pa.copy_(torch.from_numpy(pack_planes(bits_a, P).view(np.int64)))
    pb.copy_(torch.from_numpy(pack_planes(bits_b, P).view(np.int64)))
    out, chk = fenced((n, n_b, 9), torch.int64)
    ctx.contamination(ctx.records(_pack(ctx, recs, "u16"), "u16", n), P, pa, pb, out=out)
    ctx.sync()
    chk(), chk_a(), chk_b()
    assert np.array_equal(out.cpu().numpy(), sums(recs, bits_a, bits_b))
