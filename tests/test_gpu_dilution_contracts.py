"""The output contract C21 (include/amplisolve_hip.h) of ampli_dilute_records on poisoned, fenced buffers (tests/helpers.py): d_out and
d_flags are fully overwritten for n_mix mixtures -- ABSENT records and bad mixtures included -- and nothing beyond them is, the other
batches' mixtures of a larger matrix included; inputs that end where their buffers end are unchanged."""
import numpy as np
import pytest

from tests.dilution_cohorts import case, special
from tests.helpers import fenced
from tests.test_gpu_loo import _pack
from tests.test_gpu_parity import _t

pytestmark = pytest.mark.gpu


def _fenced_copy(t):
    buf, chk = fenced(tuple(t.shape), t.dtype)
    buf.copy_(t)
    return buf, chk


def _descriptors(mix):
    return np.array([[(ra & 0xFFFFFFFF) | (rb & 0xFFFFFFFF) << 32, ka, kb, key] for ra, rb, ka, kb, key in mix], dtype=np.uint64).view(np.int64)


@pytest.mark.parametrize("lay_a,lay_b", [("i32", "u16"), ("u24", "u24"), ("u16", "i32")])
@pytest.mark.parametrize("P,n_mix,kind", [(1, 1, "same"), (65, 9, "different"), (130, 9, "same")])
def test_out_and_flags_are_fully_overwritten_and_mixtures_of_a_larger_matrix(ctx, lay_a, lay_b, P, n_mix, kind):
    import torch

    A, B, mix, want, want_flags = case(P, n_mix, kind)
    if kind == "same":
        lay_b = lay_a
    # primary records only, so that the records end where their buffer ends: a row is P records
    src_a, chk_a = _fenced_copy(_pack(ctx, np.ascontiguousarray(A[0][:, :P]), lay_a))
    src_b, chk_b = _fenced_copy(_pack(ctx, np.ascontiguousarray(B[0][:, :P]), lay_b))
    ra, rb = ctx.records(src_a, lay_a, A[0].shape[0]), ctx.records(src_b, lay_b, B[0].shape[0])
    d_mix, chk_m = _fenced_copy(_t(_descriptors(mix)))
    out, chk_o = fenced((n_mix, P, 8), torch.int32)
    flags, chk_f = fenced((n_mix,), torch.int32)
    checks = (chk_a, chk_b, chk_m, chk_o, chk_f)
    before = [t.clone() for t in (src_a, src_b, d_mix)]
    lo = n_mix // 2
    ctx.dilute(ra, rb if kind == "different" else ra, P, d_mix[lo:], out=out[lo:], flags=flags[lo:])
    ctx.sync()
    [c() for c in checks]
    got, gf = out.cpu().numpy(), flags.cpu().numpy()
    assert (got[:lo] == -1).all() and (gf[:lo] == -1).all()  # the other batch's mixtures: untouched
    assert np.array_equal(got[lo:], want[lo:]) and np.array_equal(gf[lo:], want_flags[lo:])  # over the poison: every word written
    if lo:
        ctx.dilute(ra, rb if kind == "different" else ra, P, d_mix[:lo], out=out[:lo], flags=flags[:lo])
    ctx.dilute(ra, rb if kind == "different" else ra, P, d_mix[lo:], out=out[lo:], flags=flags[lo:])  # again, over its own results
    ctx.sync()
    [c() for c in checks]
    assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(flags.cpu().numpy(), want_flags)
    for t, b in zip((src_a, src_b, d_mix), before):
        assert torch.equal(t, b)  # the inputs are unchanged


def test_bad_mixtures_and_absent_records_overwrite_the_poison(ctx):
    """a bad mixture writes all its ABSENT records and its flag, and names no record to read: the chunk's buffer holds two rows, the
    mixtures name rows far outside it"""
    import torch

    recs, mix, want, want_flags = special()
    P = recs.shape[1]
    src, chk_r = _fenced_copy(_t(recs))
    r = ctx.records(src, "i32", 2)
    mix = mix[1:]  # without the long cell, which tests/test_gpu_dilution.py draws once
    d_mix, chk_m = _fenced_copy(_t(_descriptors(mix)))
    out, chk_o = fenced((len(mix), P, 8), torch.int32)
    flags, chk_f = fenced((len(mix),), torch.int32)
    flags.fill_(7)  # bits a call must clear, not OR into
    ctx.dilute(r, r, P, d_mix, out=out, flags=flags)
    ctx.sync()
    [c() for c in (chk_r, chk_m, chk_o, chk_f)]
    assert np.array_equal(out.cpu().numpy(), want[1:]) and np.array_equal(flags.cpu().numpy(), want_flags[1:])
