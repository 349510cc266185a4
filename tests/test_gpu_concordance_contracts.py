"""The output contracts of ampli_genotype_planes_records and ampli_concordance_pairs (include/amplisolve_hip.h, C11) on poisoned,
fenced buffers (tests/helpers.py): every word of the chunk's rows and every count overwritten, the bits at and beyond P zero, nothing
outside written -- the other chunks' rows of the same buffer included -- and the inputs unchanged."""
import numpy as np
import pytest

from tests.concordance_cohorts import records
from tests.concordance_model import classify, pack_planes, pair_counts, planes, words
from tests.helpers import fenced
from tests.test_gpu_loo import _pack

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("layout", ["i32", "u24", "u16"])
@pytest.mark.parametrize("P", [77, 130, 64])
def test_planes_of_a_chunk(ctx, layout, P):
    import torch

    n, lo, hi = 7, 3, 7
    W = words(P)
    recs = records(P, n, P + n)
    exp = planes(recs, P)
    buf, chk = fenced((n, 6, W), torch.int64)
    src = _pack(ctx, recs[lo:hi], layout)
    before = src.clone()
    ctx.genotype_planes(ctx.records(src, layout, hi - lo), P, out=buf[lo:hi])
    ctx.sync()
    chk()
    got = buf.cpu().numpy().view(np.uint64)
    assert (got[:lo] == np.uint64(0xFFFFFFFFFFFFFFFF)).all()          # the earlier chunk's rows: not this call's
    assert np.array_equal(got[lo:hi], exp[lo:hi])                       # every word of the chunk's rows: no poison left anywhere
    if P % 64:
        assert (got[lo:hi, :, W - 1] >> np.uint64(P % 64) == 0).all()  # the bits at and beyond P
    assert torch.equal(src, before)
    ctx.genotype_planes(ctx.records(_pack(ctx, recs[:lo], layout), layout, lo), P, out=buf[:lo])
    ctx.sync()
    chk()
    assert np.array_equal(buf.cpu().numpy().view(np.uint64), exp)


@pytest.mark.parametrize("P,n_a,n_b,same", [(65, 5, 70, False), (1000, 70, 5, False), (1000, 33, 65, False), (130, 1, 1, True), (1000, 7, 7, True),
                                            (600, 70, 70, True), (65, 130, 130, True)])
def test_counts_of_all_pairs(ctx, P, n_a, n_b, same):
    import torch

    bits = classify(records(P, 130, 1000 + P))
    pl = pack_planes(bits, P)
    a = torch.from_numpy(pl[:n_a].view(np.int64).copy()).cuda()
    b = a if same else torch.from_numpy(pl[130 - n_b:].view(np.int64).copy()).cuda()
    a0, b0 = a.clone(), b.clone()
    counts, chk = fenced((n_a, n_b, 5), torch.int32)
    L = ctx.lib
    import ctypes as C

    rc = L.ampli_concordance_pairs(ctx.h, P, C.c_void_p(a.data_ptr()), n_a, C.c_void_p(b.data_ptr()), n_b, C.c_void_p(counts.data_ptr()))
    ctx.sync()
    assert rc == 0
    chk()
    exp = pair_counts(bits[:n_a], bits[:n_b] if same else bits[130 - n_b:])
    assert np.array_equal(counts.cpu().numpy(), exp) and (exp >= 0).all()  # every count overwritten: the poison is -1
    assert torch.equal(a, a0) and torch.equal(b, b0)
