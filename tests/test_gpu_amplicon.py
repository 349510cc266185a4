"""Context.amplicon_depth / amplicon_reference / amplicon_ratio (ampli_amplicon.hip) against the definition (tests/amplicon_model.py),
exactly: np.array_equal on the int64 sums, bit for bit with NaNs matched by position on the doubles.

Depth sums: lists of 0, 1, 63, 64, 65, 129, 256, 257, 300 and 5000 entries (up to 256 a wave keeps its indices in registers, beyond it
walks the list in rounds of 64: the same wave, no other form), drawn unsorted, overlapping and with repeats, plus one contiguous run;
P = 65 and 1000; n = 1, 2, 7 and 9 (the strip of 8 rows a wave owns, -1 and +1), 31 and 33 (the 32 rows of a workgroup); every record
layout; a padded row stride; absent records; extras and an RD plane without effect; int32 fields of 2^30 and 2^31 - 1 with sums beyond
2^40; chunks into the rows of one matrix; bit-identical repeats.  Reference and ratios at N in {1, 2, 3, 4, 63, 64, 65, 257} and A in
{1, 2, 64, 65, 1000} with ties, zero rows and zero columns, a masked use, K == 0 and mad == 0.  The planted cohort end to end."""
import functools

import numpy as np
import pytest

from amplisolve_amd.api import AMPLICON_STRIP
from tests.amplicon_cohorts import N_NORMALS, planted, planted_results
from tests.amplicon_model import ABSENT, DEFAULTS, FEW, OK, depth_sums, genes, ratios, reference, same
from tests.concordance_cohorts import records
from tests.test_gpu_loo import _pack
from tests.test_gpu_parity import _t

pytestmark = pytest.mark.gpu
LENGTHS = (0, 1, 63, 64, 65, 129, 256, 257, 300, 5000, 0)
SHAPES = [(65, 1), (65, 2), (1000, AMPLICON_STRIP - 1), (1000, AMPLICON_STRIP + 1), (65, 33), (1000, 31)]
assert AMPLICON_STRIP == 8


@functools.lru_cache(maxsize=None)
def lists(P, seed=3):
    """amp_off, amp_pos: LENGTHS drawn at random from [0, P) -- unsorted, overlapping, with repeats -- then one contiguous run over the
    whole panel and a list whose only entry is the last position"""
    rng = np.random.default_rng(seed + P)
    parts = [rng.integers(0, P, n) for n in LENGTHS] + [np.arange(P), np.array([P - 1])]
    off = np.concatenate([[0], np.cumsum([len(x) for x in parts])]).astype(np.uint32)
    pos = np.concatenate(parts).astype(np.uint32)
    off.setflags(write=False)
    pos.setflags(write=False)
    return off, pos


@functools.lru_cache(maxsize=None)
def _case(P, n):
    recs = records(P, n, 16 * P + n)
    off, pos = lists(P)
    exp = depth_sums(recs, off, pos, 100)
    exp.setflags(write=False)
    return recs, off, pos, exp


@pytest.mark.parametrize("layout", ["i32", "u24", "u16"])
@pytest.mark.parametrize("P,n", SHAPES)
def test_sums_equal_the_model(ctx, layout, P, n):
    recs, off, pos, exp = _case(P, n)
    if P * n >= 5000:
        assert (recs[:, :, 0] == ABSENT).any() and (exp[:, 1:, :] > 0).any(axis=(0, 1)).all() and (exp[:, :, 3] < exp[:, :, 0]).any()
    got = ctx.amplicon_depth(ctx.records(_pack(ctx, recs, layout), layout, n), P, off, pos).cpu().numpy()
    assert got.shape == (n, len(off) - 1, 4) and got.dtype == np.int64 and np.array_equal(got, exp)


@pytest.mark.parametrize("cov", [0, 1, 99, 101, 30000])
def test_the_cut_off(ctx, cov):
    recs, off, pos, _ = _case(1000, 7)
    got = ctx.amplicon_depth(ctx.records(_pack(ctx, recs, "u16"), "u16", 7), 1000, off, pos, cov=cov).cpu().numpy()
    assert np.array_equal(got, depth_sums(recs, off, pos, cov))


@pytest.mark.parametrize("layout", ["i32", "u24", "u16"])
def test_a_padded_row_stride(ctx, layout):
    P, n, pad = 65, 9, 7
    recs = records(P + pad, n, 21)  # the pad holds records too: they must not be read in place of the next row's
    off, pos = lists(P)
    got = ctx.amplicon_depth(ctx.records(_pack(ctx, recs, layout), layout, n, row_stride=P + pad), P, off, pos).cpu().numpy()
    assert np.array_equal(got, depth_sums(recs[:, :P], off, pos))


@pytest.mark.parametrize("layout", ["i32", "u24"])
def test_extras_and_an_rd_plane_do_not_matter(ctx, layout):
    P, n, E = 130, 7, 9
    recs = records(P, n, 77, extras=E)
    rng = np.random.default_rng(4)
    dup_off = np.concatenate([[0], np.cumsum(np.isin(np.arange(P), rng.choice(P, E, replace=False)))]).astype(np.uint32)
    ext_pos = np.repeat(np.arange(P), np.diff(dup_off.astype(np.int64))).astype(np.uint32)
    rd = np.where(rng.random((n, P + E)) < 0.3, 12345, ABSENT).astype(np.int32)
    full = ctx.records(_pack(ctx, recs, layout), layout, n, E=E, dup_off=_t(dup_off), ext_pos=_t(ext_pos), rd=_t(rd[:, :P]), rd_ext=_t(rd[:, P:]))
    plain = ctx.records(_pack(ctx, recs[:, :P], layout), layout, n)
    off, pos = lists(P)
    a, b = ctx.amplicon_depth(full, P, off, pos).cpu().numpy(), ctx.amplicon_depth(plain, P, off, pos).cpu().numpy()
    assert np.array_equal(a, b) and np.array_equal(a, depth_sums(recs[:, :P], off, pos))


def test_i32_fields_of_two_to_the_thirty_and_beyond(ctx):
    P, n = 1000, 9
    big, top = 1 << 30, (1 << 31) - 1
    menu = np.array([[big, 0, 0, 1 << 25, big, 0, 0, 1 << 25], [top, top, top, top, top, top, top, top], [0, top, top >> 5, 0, 0, top, 0, 7],
                     [99, 0, 0, 0, top, top, 0, 0], [3, 0, 5, top, 0, 0, 0, 99], [ABSENT, top, 0, 0, top, 0, 0, 0]], np.int64).astype(np.int32)
    recs = menu[np.random.default_rng(30).integers(0, len(menu), (n, P))]
    off, pos = lists(P)
    exp = depth_sums(recs, off, pos)
    assert (exp[:, 9, 1:3] > 1 << 40).all() and (recs == top).any() and (recs == big).any()
    got = ctx.amplicon_depth(ctx.records(_t(recs), "i32", n), P, off, pos).cpu().numpy()
    assert np.array_equal(got, exp)


@pytest.mark.parametrize("layout", ["i32", "u24", "u16"])
def test_chunks_into_the_rows_of_one_matrix(ctx, layout):
    import torch

    P, n, cuts = 1000, 31, (0, 7, 8, 24, 31)
    recs, off, pos, exp = _case(P, n)
    d_off, d_pos = _t(off.astype(np.int32)), _t(pos.astype(np.int32))
    buf = torch.full((n, len(off) - 1, 4), -1, dtype=torch.int64, device=ctx.device)
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        out = ctx.amplicon_depth(ctx.records(_pack(ctx, recs[lo:hi], layout), layout, hi - lo), P, d_off, d_pos, out=buf[lo:hi])
        assert out.data_ptr() == buf[lo:hi].data_ptr()
    assert np.array_equal(buf.cpu().numpy(), exp)


def test_two_runs_are_bit_identical(ctx):
    recs, off, pos, exp = _case(1000, 31)
    rec = ctx.records(_pack(ctx, recs, "u24"), "u24", 31)
    one = ctx.amplicon_depth(rec, 1000, off, pos).cpu().numpy().tobytes()
    two = ctx.amplicon_depth(rec, 1000, off, pos).cpu().numpy().tobytes()
    assert one == two == exp.tobytes()


# ---- reference and ratios ----

@functools.lru_cache(maxsize=None)
def matrix(N, A, seed=0):
    """sums int64 [N, A, 4] with ties (few distinct depths, equal rows), zero rows (T == 0) and zero columns (DARK); use with a masked
    third"""
    rng = np.random.default_rng(1000 * N + A + seed)
    d = rng.choice([0, 1, 2, 3, 5, 40, 1000, 65534 * 130, 1 << 40], size=(N, A)) * rng.integers(1, 4, (N, 1))
    d[:, rng.random(A) < 0.15] = 0
    if N > 2:
        d[rng.random(N) < 0.1] = 0
        d[N // 2] = d[0]
    sums = np.zeros((N, A, 4), np.int64)
    sums[:, :, 1] = d // 2
    sums[:, :, 2] = d - d // 2
    sums[:, :, 0] = rng.integers(0, 300, (N, A))
    sums[:, :, 3] = rng.integers(0, 300, (N, A))
    use = (rng.random(A) < 0.7).astype(np.uint8)
    if A <= 2:
        use[:] = 1
    sums.setflags(write=False)
    use.setflags(write=False)
    return sums, use


def _reference_equal(got, exp):
    assert np.array_equal(got["total"].cpu().numpy(), exp["total"])
    assert np.array_equal(got["status"].cpu().numpy(), exp["status"])
    assert same(got["med"].cpu().numpy(), exp["med"]) and same(got["mad"].cpu().numpy(), exp["mad"])


def _ratio_equal(got, exp):
    assert np.array_equal(got["total"].cpu().numpy(), exp["total"]) and np.array_equal(got["k"].cpu().numpy(), exp["k"])
    assert same(got["centre"].cpu().numpy(), exp["centre"])
    assert same(got["ratio"].cpu().numpy(), exp["ratio"]) and same(got["z"].cpu().numpy(), exp["z"])


@pytest.mark.parametrize("A", [1, 2, 64, 65, 1000])
@pytest.mark.parametrize("N", [1, 2, 3, 4, 63, 64, 65, 257])
def test_reference_and_ratios_equal_the_model(ctx, N, A):
    sums, use = matrix(N, A)
    d_sums, d_use = _t(sums), _t(use)
    for min_normals in (1, max(1, N // 2)):
        exp = reference(sums, use, min_normals)
        got = ctx.amplicon_reference(d_sums, d_use, min_normals)
        _reference_equal(got, exp)
        _ratio_equal(ctx.amplicon_ratio(d_sums, d_use, got), ratios(sums, use, exp))
    if N >= 63 and A >= 64:
        st = exp["status"]
        assert (exp["total"] == 0).any() and (st == OK).any() and (st != OK).any()
        assert exp["n_eff"] < N


def test_few_normals_k_zero_and_a_mask_of_zeros(ctx):
    sums, use = matrix(65, 64)
    d_sums = _t(sums)
    exp = reference(sums, use, 66)
    got = ctx.amplicon_reference(d_sums, _t(use), 66)
    assert (exp["status"] == FEW).all()
    _reference_equal(got, exp)
    r = ratios(sums, use, exp)
    assert (r["k"] == 0).all() and (r["total"] > 0).any() and np.isnan(r["ratio"]).all()   # K == 0 with T > 0
    _ratio_equal(ctx.amplicon_ratio(d_sums, _t(use), got), r)
    zero = np.zeros_like(use)
    exp = reference(sums, zero, 1)
    got = ctx.amplicon_reference(d_sums, _t(zero), 1)
    assert exp["n_eff"] == 0 and np.isnan(exp["med"]).all()                                  # nobody is included
    _reference_equal(got, exp)
    _ratio_equal(ctx.amplicon_ratio(d_sums, _t(zero), got), ratios(sums, zero, exp))
    # more than half of the normals alike: mad == 0 under status OK, z is NaN
    a, b, c = np.flatnonzero(reference(sums, use, 1)["total"] > 0)[:3]
    alike = np.ascontiguousarray(sums[[a, b, a, c, a]])
    exp = reference(alike, use, 1)
    got = ctx.amplicon_reference(_t(alike), _t(use), 1)
    assert ((exp["status"] == OK) & (exp["mad"] == 0)).any() and exp["n_eff"] == 5
    _reference_equal(got, exp)
    _ratio_equal(ctx.amplicon_ratio(_t(alike), _t(use), got), ratios(alike, use, exp))
    # other samples than the reference's
    other, _ = matrix(7, 64, seed=5)
    exp = reference(sums, use, 5)
    got = ctx.amplicon_reference(d_sums, _t(use), 5)
    _ratio_equal(ctx.amplicon_ratio(_t(other), _t(use), got), ratios(other, use, exp))


def test_planted_cohort_end_to_end(ctx):
    c, r = planted(), planted_results()
    n, P = c["recs"].shape[0], c["P"]
    sums = ctx.amplicon_depth(ctx.records(_pack(ctx, c["recs"], "u16"), "u16", n), P, c["amp_off"], c["amp_pos"], cov=DEFAULTS["coverage_cutoff"])
    assert np.array_equal(sums.cpu().numpy(), r["sums"])
    use = _t(c["use"])
    ref = ctx.amplicon_reference(sums[:N_NORMALS].contiguous(), use, DEFAULTS["min_normals"])
    _reference_equal(ref, r["ref"])
    rat = ctx.amplicon_ratio(sums, use, ref)
    _ratio_equal(rat, r["rat"])
    kw = {k: DEFAULTS[k] for k in ("min_amplicons", "gain_ratio", "loss_ratio", "z_cutoff")}
    g = genes(rat["ratio"].cpu().numpy(), rat["z"].cpu().numpy(), ref["status"].cpu().numpy(), c["gene_of"], **kw)
    assert {k: v[3] for k, v in g.items()} == {k: v[3] for k, v in r["genes"].items()}
