"""The output contracts of ampli_dispersion_records and ampli_dispersion_finalize (include/amplisolve_hip.h, C10) on poisoned, fenced
buffers (tests/helpers.py): the planes overwritten or added to, the sample arrays fully overwritten or absent, the counters added to,
nothing written outside, and bad arguments refused with AMPLI_E_INVALID before anything is written."""
import ctypes as C

import numpy as np
import pytest

from tests.dispersion_cohorts import cohort_and_model
from tests.dispersion_model import FEW
from tests.helpers import fenced
from tests.test_gpu_loo import _pack
from tests.test_gpu_parity import _t

pytestmark = pytest.mark.gpu
P, S, COV = 130, 3, 100
E_INVALID = -1


def _setup(ctx, layout="u16", cuts=(0, 2, 3)):
    (recs, E, dup_off, ext_pos, rd), exp = cohort_and_model(P, S, 77, True, False, True, COV)
    acc0 = ctx.new_acc(P)
    chunks = []
    for ci in range(len(cuts) - 1):
        lo, hi = cuts[ci], cuts[ci + 1]
        rec = ctx.records(_pack(ctx, recs[lo:hi], layout), layout, hi - lo, E=E, dup_off=_t(dup_off), ext_pos=_t(ext_pos))
        ctx.error_reduce_records(rec, P, acc0, 0.0, COV, first_sample=lo, accumulate=ci > 0, summary=True)
        chunks.append((lo, hi, rec))
    return chunks, acc0, exp


def _close(a, b, scale):
    return (np.abs(a - b) <= 1e-12 * scale).all()


@pytest.mark.parametrize("layout", ["i32", "u24", "u16"])
def test_planes_sample_arrays_and_counters(ctx, layout):
    import torch

    chunks, acc0, exp = _setup(ctx, layout)
    assert (exp["status"] != FEW).sum() > 100 and (exp["status"] == FEW).sum() > 100
    K = exp["K"].astype(np.float64)
    x2, x2_chk = fenced((2, 4, P), torch.float64)
    rinv, rinv_chk = fenced((2, 4, P), torch.float64)
    fences = [x2_chk, rinv_chk]
    got_terms = []
    for i, (lo, hi, rec) in enumerate(chunks):
        sx, sx_chk = fenced((hi - lo,), torch.float64)
        se, se_chk = fenced((hi - lo,), torch.float64)
        stm, st_chk = fenced((hi - lo,), torch.int64)
        before = x2.cpu().numpy().copy()
        ctx.dispersion_records(rec, P, acc0, COV, x2, rinv, accumulate=i > 0, sample_x2=sx, sample_expect=se, sample_terms=stm)
        ctx.sync()
        for chk in fences + [sx_chk, se_chk, st_chk]:
            chk()
        assert not torch.isnan(x2).any() and not torch.isnan(rinv).any()           # overwritten: no poison left (0xFF.. is NaN)
        assert not torch.isnan(sx).any() and not torch.isnan(se).any() and (stm >= 0).all()
        if i > 0:  # added to: nothing shrinks, FEW cells stay 0
            assert (x2.cpu().numpy() >= before).all()
        got_terms.append(stm.cpu().numpy())
        assert np.array_equal(got_terms[-1], exp["sample_terms"][lo:hi])
        assert _close(sx.cpu().numpy(), exp["sample_x2"][lo:hi], 100 * (1 + exp["sample_x2"][lo:hi] + exp["sample_scale"][lo:hi]))
    assert _close(x2.cpu().numpy(), exp["x2"], 1 + K + exp["x2"]) and _close(rinv.cpu().numpy(), exp["rinv"], exp["rinv"])
    # a second round with accumulate: exactly twice the first chunk's share on top -- the planes are ADDED to
    once = x2.cpu().numpy().copy()
    lo, hi, rec = chunks[0]
    first, _ = fenced((2, 4, P), torch.float64)
    first_r, _ = fenced((2, 4, P), torch.float64)
    ctx.dispersion_records(rec, P, acc0, COV, first, first_r, accumulate=False)  # the NULL sample arrays
    ctx.dispersion_records(rec, P, acc0, COV, x2, rinv, accumulate=True)
    ctx.sync()
    for chk in fences:
        chk()
    assert np.array_equal(x2.cpu().numpy(), once + first.cpu().numpy())
    # finalize: z, phi and status overwritten, the four counters added to
    ctx.dispersion_records(chunks[0][2], P, acc0, COV, x2, rinv, accumulate=False)
    ctx.dispersion_records(chunks[1][2], P, acc0, COV, x2, rinv, accumulate=True)
    z, z_chk = fenced((2, 4, P), torch.float64)
    phi, phi_chk = fenced((2, 4, P), torch.float32)
    status, s_chk = fenced((2, 4, P), torch.uint8)
    counts, c_chk = fenced((4,), torch.int64, poison=0)
    counts.copy_(torch.tensor([1000, 2000, 3000, 4000], dtype=torch.int64))
    for rounds in (1, 2):
        ctx.dispersion_finalize(P, acc0, x2, rinv, 4.0, z, phi, status, counts)
        ctx.sync()
        for chk in (z_chk, phi_chk, s_chk, c_chk, x2_chk, rinv_chk):
            chk()
        assert not torch.isnan(z).any() and not torch.isnan(phi).any()
        assert np.array_equal(status.cpu().numpy() & 7, exp["status"] & 7)
        assert counts.cpu().numpy().tolist() == [1000 + rounds * int(exp["counts"][0]), 2000 + rounds * int(exp["counts"][1]),
                                                 3000 + rounds * int(exp["counts"][2]), 4000 + rounds * int(exp["counts"][3])]
    assert _close(z.cpu().numpy(), exp["z"], 1 + K + np.abs(exp["z"]))


def test_bad_arguments_are_refused_before_anything_is_written(ctx):
    import torch

    chunks, acc0, exp = _setup(ctx)
    rec = chunks[0][2]
    n = rec.n_samples
    x2, x2_chk = fenced((2, 4, P), torch.float64)
    rinv, rinv_chk = fenced((2, 4, P), torch.float64)
    sx, sx_chk = fenced((n,), torch.float64)
    se, se_chk = fenced((n,), torch.float64)
    stm, st_chk = fenced((n,), torch.int64)
    z, z_chk = fenced((2, 4, P), torch.float64)
    phi, phi_chk = fenced((2, 4, P), torch.float32)
    status, s_chk = fenced((2, 4, P), torch.uint8)
    counts, c_chk = fenced((4,), torch.int64)
    other = ctx.new_acc(P + 1)
    L = ctx.lib
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    A = C.byref(acc0.struct)

    def records(h=ctx.h, r=rec, P_=P, acc=A, cov=COV, a=x2, b=rinv, sx_=sx, se_=se, st_=stm):
        return L.ampli_dispersion_records(h, C.byref(r) if r is not None else None, P_, acc, cov, p(a), p(b), 0, p(sx_), p(se_), p(st_))

    def finalize(h=ctx.h, P_=P, acc=A, a=x2, b=rinv, cut=4.0, z_=z, phi_=phi, s_=status, c_=counts):
        return L.ampli_dispersion_finalize(h, P_, acc, p(a), p(b), cut, p(z_), p(phi_), p(s_), p(c_))

    no_dup = ctx.records(rec._keep[0], "u16", n, E=rec.E)  # E > 0 without dup_off
    bad = [records(h=None), records(r=None), records(P_=0), records(P_=-5), records(acc=None), records(acc=C.byref(other.struct)), records(cov=0),
           records(a=None), records(b=None), records(sx_=None), records(se_=None), records(st_=None), records(sx_=None, se_=None), records(r=no_dup),
           records(a=x2.view(torch.uint8)[4:12]),
           finalize(h=None), finalize(P_=0), finalize(acc=None), finalize(acc=C.byref(other.struct)), finalize(a=None), finalize(b=None),
           finalize(cut=float("nan")), finalize(z_=None), finalize(phi_=None), finalize(s_=None), finalize(c_=None)]
    ctx.sync()
    assert bad == [E_INVALID] * len(bad), bad
    assert L.ampli_last_error(ctx.h).decode() != ""
    for t, chk in ((x2, x2_chk), (rinv, rinv_chk), (sx, sx_chk), (se, se_chk), (stm, st_chk), (z, z_chk), (phi, phi_chk), (status, s_chk), (counts, c_chk)):
        chk()
        assert (chk.raw == 0xFF).all()  # nothing written, the payload included
    assert records() == 0 and finalize(c_=torch.zeros(4, dtype=torch.int64, device=ctx.device)) == 0  # and the good call passes
    ctx.sync()
