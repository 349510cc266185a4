"""The three device scorers over the whole int32 domain, against the oracle's literal scorer (orc.score_batch, bit-identical to the
reference's compiled functions): ctx.score_batch (ampli_poisson_score, the literal form), ctx.score_dense_batch
(ampli_poisson_score_dense, the all-scores mode: lgamma table, closed form / convergents of the continued fraction) and
ctx.drain_score_batch (ampli_drain_p, the drain's division-free series on the same table; only on points with 0 < m < k).

The points are those of the host's sweeps (tests/scorer_grids.py; tests/test_math_host.py runs all of them at 1e-11): each grid
subsampled to 150 000 points with a fixed seed, plus the explicit edges -- the lgamma table's last entry, counts and depths from
2^24 - 1 to INT32_MAX, the bound of the closed form, k = 0, rd = 0, negative counts, depths and errors.  The device's
exp / log / log10 / frexp / ldexp / fma are ocml's, not glibc's, so none of this follows from the host's sweep.  The checks are
scorer_grids.compare_with_oracle's: NaN pattern and special codes, p within 1e-6 (absolute, and relative above 1e-10), Q within
1e-5 where it is not clamped, the gate decisions outside 1e-6 of a gate, at most 0.1 % of the points inside such a band.

The points with k = INT32_MAX were first sent to a GPU after tests/csrc/scorer_domain_main.cpp had run clean under the address
and undefined-behaviour sanitizers on the host (before, k + 1 wrapped and indexed far below the table).

Points per test: 150 000 of the drain's grid (291 600), 150 000 of the all-scores grid (491 336), 701 edge points; the drain's
scorer sees the 150 000 / 64 834 / 269 of them that lie in its domain.  No point of either grid lies within 1e-6 of a gate (in-band
share 0, subsampled and whole; 0.1 % is allowed).

Measured on an MI355X, worst relative error of p (> 1e-10) per decade of the depth; every run prints these lines:
  depth   literal  dense (p from Q)  drain      literal  dense    drain      (left: drain's grid; right: all-scores grid)
  1e0                                           7.8e-16  2.8e-14  2.8e-14
  1e1     1.8e-14  4.1e-13           4.1e-13    1.8e-14  4.1e-13  4.1e-13
  1e2     2.3e-13  9.9e-13           9.9e-13    1.9e-13  1.9e-13  1.3e-13
  1e3     2.1e-13  2.4e-13           2.4e-13    2.7e-13  2.7e-13  1.0e-13
  1e4     7.3e-12  1.8e-09           1.8e-09    1.5e-11  1.5e-11  1.5e-11
  1e5     2.9e-11  2.9e-11           2.9e-11    1.8e-12  1.8e-12  1.8e-12
  1e6     4.7e-10  4.7e-10           4.7e-10    3.6e-12  3.6e-12  3.6e-12
  1e7     7.5e-09  7.5e-09           7.5e-09    1.5e-08  1.5e-08  1.5e-08
  1e8..   3.7e-09  3.7e-09           3.7e-09    9.5e-07  9.5e-07  9.5e-07
Edge points: at most 3.8e-14.  The whole grids, measured once: 1.2e-7 (drain's) and 9.5e-7 (all-scores), nothing beyond 1e-6.
9.5e-7 is 2^-20: at s ~ z ~ 10^9 the exponent s ln z - z - lgamma(s + 1) is made of terms of 2e10, whose ulp is 2^-19, so one
differently rounded log moves p by that much -- in the literal form as in the two others.  The contract's 1e-6 on p holds up to
these depths without margin; it is not a property of the table forms.
"""
import functools

import numpy as np
import pytest

from oracle import pyoracle as orc
from tests import scorer_grids

pytestmark = pytest.mark.gpu


def _t(x):
    import torch

    return torch.from_numpy(np.array(x)).cuda()  # a copy: the shared points are read-only


@functools.lru_cache(maxsize=None)
def _points(which):
    """(k, rd, err, oracle Q, oracle p) of one set, computed once and shared by the three scorers' tests (read-only)"""
    if which == "drain_grid":
        k, rd, e = scorer_grids.subsample(*scorer_grids.drain_grid())
    elif which == "dense_grid":
        k, rd, e = scorer_grids.subsample(*scorer_grids.dense_grid())
    else:
        k1, rd1, e1, above = scorer_grids.table_end_points()
        q1, _ = orc.score_batch(k1, rd1, e1)
        assert above.any() and (~above).any() and ((q1[above] > 5) & (q1[above] < 100)).all()
        k2, rd2, e2 = scorer_grids.edge_points()
        k, rd, e = np.concatenate([k1, k2]), np.concatenate([rd1, rd2]), np.concatenate([e1, e2])
    qo, po = orc.score_batch(k, rd, e)
    for a in (k, rd, e, qo, po):
        a.setflags(write=False)
    return k, rd, e, qo, po


SETS = ("drain_grid", "dense_grid", "edges")


@pytest.mark.parametrize("which", SETS)
def test_literal_scorer_over_the_domain(ctx, which):
    k, rd, e, qo, po = _points(which)
    assert k.size <= scorer_grids.GPU_POINTS and (k == scorer_grids.INT32_MAX).any()
    q, p = ctx.score_batch(_t(k), _t(rd), _t(e))
    scorer_grids.compare_with_oracle(f"score_batch/{which}", k, rd, e, qo, po, q.cpu().numpy(), p.cpu().numpy())
    assert ctx.flags() == 0


@pytest.mark.parametrize("which", SETS)
def test_dense_scorer_over_the_domain(ctx, which):
    k, rd, e, qo, po = _points(which)
    q = ctx.score_dense_batch(_t(k), _t(rd), _t(e)).cpu().numpy()
    scorer_grids.compare_with_oracle(f"score_dense_batch/{which}", k, rd, e, qo, po, q)
    assert ctx.flags() == 0


@pytest.mark.parametrize("which", SETS)
def test_drain_scorer_over_its_domain(ctx, which):
    k, rd, e, qo, po = _points(which)
    d = scorer_grids.in_drain_domain(k, rd, e)
    assert d.sum() >= (50_000 if which != "edges" else 40)
    assert (k[d] == scorer_grids.INT32_MAX).any() and (k[d] > scorer_grids.LGTAB).any() and (k[d] < scorer_grids.LGTAB - 1).any()
    k, rd, qo, po = k[d], rd[d], qo[d], po[d]
    e = np.where(e[d] == 0, np.float32(0.0010008), e[d]).astype(np.float32)  # the drain is handed the effective error
    q, p = ctx.drain_score_batch(_t(k), _t(rd), _t(e))
    scorer_grids.compare_with_oracle(f"drain_score_batch/{which}", k, rd, e, qo, po, q.cpu().numpy(), p.cpu().numpy())
    assert ctx.flags() == 0


def test_drain_probe_is_the_hosts_probe_on_small_counts(ctx):
    """ampli_drain_score_batch has the semantics of ampli_host_drain_score_batch: the same q and p to rounding on a 2000x panel's items,
    and either output may be left out"""
    import ctypes as C

    import torch

    from amplisolve_amd import host_lib

    rng = np.random.default_rng(3)
    rd = rng.integers(500, 4000, 3001).astype(np.int32)  # 3001: more than one block, not a multiple of 256
    e = rng.choice(np.array([0.002, 0.0005, 0.01], np.float32), rd.size)
    k = (np.floor(rd * e.astype(np.float64)) + rng.integers(1, 12, rd.size)).astype(np.int32)
    qh, ph = np.empty(k.size), np.empty(k.size)
    host_lib().ampli_host_drain_score_batch(k.ctypes.data_as(C.c_void_p), rd.ctypes.data_as(C.c_void_p), e.ctypes.data_as(C.c_void_p), k.size,
                                            qh.ctypes.data_as(C.c_void_p), ph.ctypes.data_as(C.c_void_p))
    dk, drd, de = _t(k), _t(rd), _t(e)
    q, p = ctx.drain_score_batch(dk, drd, de)
    assert np.max(np.abs(p.cpu().numpy() - ph) / ph) <= 1e-6 and np.max(np.abs(q.cpu().numpy() - qh)) <= 1e-5
    only_q = torch.full((k.size,), -7.0, dtype=torch.float64, device="cuda")
    ctx._check(ctx.lib.ampli_drain_score_batch(ctx.h, dk.data_ptr(), drd.data_ptr(), de.data_ptr(), k.size, only_q.data_ptr(), None))
    assert torch.equal(only_q, q)
