"""Context.fdr_adjust (csrc/ampli_fdr.hip: the key kernel, the radix sort's histogram / scan / stable scatter, the running maximum and the
binary-search lookup) against the definition (tests/fdr_model.py) on planes built directly in torch (tests/fdr_planes.py): m and rank
exact; the tested mask, the sign, +0 and NA exact; |dA| <= 1e-5; two runs, a row alone and a row in a batch give the same bytes."""
import numpy as np
import pytest

from tests import fdr_model as fm
from tests import fdr_planes as fp
from tests.test_gpu_parity import _t

pytestmark = pytest.mark.gpu
NA = np.float32(fm.NA)


def _run(ctx, s, two_sided, rank=True, **kw):
    out = ctx.fdr_adjust(s, two_sided, rank=rank, **kw)
    ctx.sync()
    return [t.cpu().numpy() for t in out]


@pytest.mark.parametrize("two_sided", [False, True])
@pytest.mark.parametrize("P", fp.edges())
def test_fdr_equals_the_model(ctx, P, two_sided):
    """one row per kind of plane (random scores, five values, all 100, all zero, all NA, one tested cell, keys that differ in one radix
    digit only, -0.0f among positives), adjusted in batches of 1, 3, 5 and 3 rows"""
    s, A, m, R = fp.case(P, two_sided)
    d_s = _t(s.copy())  # the shared case is read-only
    worst = 0.0
    for lo, hi in fp.BATCHES:
        a, mm, r = _run(ctx, d_s[lo:hi], two_sided)
        worst = max(worst, fm.compare(a, mm, r, A[lo:hi], m[lo:hi], R[lo:hi]))
    print("P", P, "two_sided", two_sided, "worst |dA|", worst, "m", m.tolist())
    assert d_s.cpu().numpy().tobytes() == s.tobytes()  # the plane is never written


@pytest.mark.parametrize("two_sided", [False, True])
@pytest.mark.parametrize("P", [65, fp.TILE_KEYS // 4 + 1, 2 * (fp.TILE_KEYS // 4) + 1])
def test_same_bytes_again_alone_and_without_ranks(ctx, P, two_sided):
    s, A, m, R = fp.case(P, two_sided)
    d_s = _t(s[:5].copy())
    a, mm, r = _run(ctx, d_s, two_sided)
    a2, mm2, r2 = _run(ctx, d_s, two_sided)
    assert a.tobytes() == a2.tobytes() and mm.tobytes() == mm2.tobytes() and r.tobytes() == r2.tobytes()
    for row in range(5):  # a row adjusted alone: the bytes it has in the batch of five
        a1, m1, r1 = _run(ctx, d_s[row:row + 1], two_sided)
        assert a1.tobytes() == a[row:row + 1].tobytes() and m1[0] == mm[row] and r1.tobytes() == r[row:row + 1].tobytes(), row
    a3, mm3 = _run(ctx, d_s, two_sided, rank=False)  # d_rank NULL
    assert a3.tobytes() == a.tobytes() and mm3.tobytes() == mm.tobytes()


def test_a_workspace_of_the_callers_and_outputs_of_the_callers(ctx):
    import torch

    P = 1000
    s, A, m, R = fp.case(P, False)
    d_s = _t(s[:3].copy())
    work = torch.empty((ctx.fdr_workspace_bytes(3, P),), dtype=torch.uint8, device="cuda")
    a, mm, r = (torch.empty((3, P, 4), dtype=torch.float32, device="cuda"), torch.empty((3,), dtype=torch.int32, device="cuda"),
                torch.empty((3, P, 4), dtype=torch.int32, device="cuda"))
    out = ctx.fdr_adjust(d_s, False, a=a, m=mm, rank=r, work=work)
    ctx.sync()
    assert out[0] is a and out[1] is mm and out[2] is r
    fm.compare(a.cpu().numpy(), mm.cpu().numpy(), r.cpu().numpy(), A[:3], m[:3], R[:3])
    assert ctx.fdr_workspace_bytes(1, P) * 3 == ctx.fdr_workspace_bytes(3, P) and ctx.fdr_workspace_bytes(3, P) >= 3 * 2 * 4 * P * 4
    assert ctx.fdr_workspace_bytes(0, P) == 0 and ctx.fdr_workspace_bytes(1, 0) == 0 and ctx.fdr_workspace_bytes(1, 1 << 29) == 0


# ---- planes of the project's own scorers ---------------------------------------------------------------------------------------------------

def test_planes_of_nb_score_and_pair_score(ctx):
    """a planted dispersion cohort scored on the device -- the exact Poisson tail, the fitted omega, and the paired test of its tumours
    -- adjusted on the device and checked against the model on the downloaded plane"""
    from tests.overdispersion_cohorts import planted_and_fit
    from tests.test_gpu_loo import _pack
    from tests.test_gpu_overdispersion import PLANTED, _panel

    (normals, tumours, ref, over, variants), dm, s2_exp, _, _ = planted_and_fit(**PLANTED)
    P, T = normals.shape[1], tumours.shape[0]
    table, acc0, disp, s2, omega = _panel(ctx, normals, P)
    rt = ctx.records(_pack(ctx, tumours, "u16"), "u16", T)
    d_ref = _t(ref)
    planes = [(ctx.nb_score(rt, P, table.thr, d_ref, None, 100), False), (ctx.nb_score(rt, P, table.thr, d_ref, omega, 100), False)]
    pairs = _t(np.array([[i, j] for i in range(T) for j in range(T) if i != j], np.int32))
    planes.append((ctx.pair_score(rt, rt, P, pairs, d_ref, 100), True))
    for q, two_sided in planes:
        a, m, r = _run(ctx, q, two_sided)
        worst = fm.check(a, m, r, q.cpu().numpy(), two_sided)
        found = int((np.abs(a[a != NA]) >= 13.0).sum())
        print("two_sided", two_sided, "rows", q.shape[0], "m", m.tolist(), "cells with |A| >= 13:", found, "worst |dA|", worst)
        assert (m > 0).all() and found > 0
