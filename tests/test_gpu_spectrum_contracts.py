"""The output contract C16 of ampli_spectrum_records (include/amplisolve_hip.h) on poisoned, fenced buffers (tests/helpers.py): every cell
of the chunk's rows written whatever the matrix held -- the nine zeros of a class without a position included -- and nothing written
outside: the other chunks' rows keep what they held.  What is read ends where its buffer ends: the records, the reference codes and the
classes.  Both forms: one segment (plain stores over the poison) and several (the call clears its rows, the segments add)."""
import numpy as np
import pytest

from tests.helpers import fenced
from tests.spectrum_model import CLASSES, class_sums
from tests.test_gpu_loo import _pack
from tests.test_gpu_spectrum import STRIP, classes, spec_records

pytestmark = pytest.mark.gpu


def _fenced_copy(t):
    buf, chk = fenced(tuple(t.shape), t.dtype)
    buf.copy_(t)
    return buf, chk


@pytest.mark.parametrize("layout", ["i32", "u24", "u16"])
@pytest.mark.parametrize("P,segmented", [(65, False), (1000, False), (40001, True)])
def test_sums_of_a_chunk(ctx, layout, P, segmented):
    import torch

    n, lo, hi = 2 * STRIP + 3, STRIP + 1, 2 * STRIP + 3  # the chunk: a strip and a partial one, behind an earlier chunk's rows
    recs, ref = spec_records(P, n, P + n)
    cls = np.where(classes(P, CLASSES, P) == 11, 12, classes(P, CLASSES, P)).astype(np.uint8)  # class 11 has no position
    exp = class_sums(recs, ref, cls, CLASSES)
    assert not exp[:, 11].any() and exp[:, 12].any()
    src, chk_src = _fenced_copy(_pack(ctx, recs[lo:hi], layout))  # the records end where their buffer ends
    d_ref, chk_ref = _fenced_copy(torch.from_numpy(ref.copy()))
    d_cls, chk_cls = _fenced_copy(torch.from_numpy(cls.copy()))
    buf, chk = fenced((n, CLASSES, 9), torch.int64)
    before = src.clone()
    ctx.spectrum(ctx.records(src, layout, hi - lo), P, d_ref, d_cls, CLASSES, out=buf[lo:hi])
    ctx.sync()
    assert (ctx.last_spectrum_segments() > 1) == segmented
    chk(), chk_src(), chk_ref(), chk_cls()
    got = buf.cpu().numpy()
    assert (got[:lo] == -1).all()                   # the earlier chunk's rows: not this call's
    assert np.array_equal(got[lo:hi], exp[lo:hi])   # every sum of the chunk's rows, the empty class's zeros included: no poison left
    assert torch.equal(src, before) and np.array_equal(d_ref.cpu().numpy(), ref) and np.array_equal(d_cls.cpu().numpy(), cls)
    ctx.spectrum(ctx.records(_pack(ctx, recs[:lo], layout), layout, lo), P, d_ref, d_cls, CLASSES, out=buf[:lo])
    ctx.spectrum(ctx.records(src, layout, hi - lo), P, d_ref, d_cls, CLASSES, out=buf[lo:hi])  # again, over its own results
    ctx.sync()
    chk()
    assert np.array_equal(buf.cpu().numpy(), exp)


@pytest.mark.parametrize("P", [130, 70000])
def test_the_sums_end_where_their_buffer_ends(ctx, P):
    """the last row's last class is the last 72 bytes of the payload; with every position skipped, every cell is still written"""
    import torch

    n = STRIP
    recs, ref = spec_records(P, n, 5)
    buf, chk = fenced((n, 128, 9), torch.int64)
    rec = ctx.records(_pack(ctx, recs, "u16"), "u16", n)
    ctx.spectrum(rec, P, ref, np.full(P, 255, np.uint8), 128, out=buf)
    ctx.sync()
    chk()
    assert (buf.cpu().numpy() == 0).all()
    chk.repoison()
    last = np.full(P, 127, np.uint8)
    ctx.spectrum(rec, P, ref, last, 128, out=buf)
    ctx.sync()
    chk()
    got = buf.cpu().numpy()
    assert np.array_equal(got, class_sums(recs, ref, last, 128)) and got[:, 127, 0].min() > 0 and not got[:, :127].any()
