"""Context.exceedance (ampli_exceedance.hip) against the definition (tests/exceedance_model.py), exactly: np.array_equal on the unsigned
16-bit counts of both outputs.

Shapes (P, n_t, n_n) = (1, 1, 1), (63, 1, 2), (64, 2, 3), (65, 3, 5), (130, 3, 17), (1000, 5, 33) with all nine pairs of record layouts
and (1000, 33, 70) with a mixed pair: one lane, a partial tile, a tile, a tile and one lane, several tiles, several strips of normals and
several row groups of tumours.  n_n around one and two strips, n_t around the row group.  A padded row stride; absent records; extras
and an RD plane without effect; int32 fields of 2^30 and 2^31 - 1; the normals in 1, 2 and 5 chunks into the same outputs, NA staying NA;
skip_same_index with the same chunk on both sides; bit-identical repeats; the cut-offs at their edges; the planted cohort end to end."""
import functools

import numpy as np
import pytest

from amplisolve_amd.api import EXCEEDANCE_MAX_NORMALS, EXCEEDANCE_NA, EXCEEDANCE_ROWS, EXCEEDANCE_STRIP
from tests.exceedance_cohorts import CAND, N_NORMALS, planted, planted_results
from tests.exceedance_model import ABSENT, DEFAULTS, MAX_NORMALS, NA, candidates, exceedance
from tests.test_gpu_loo import _pack
from tests.test_gpu_parity import _t

pytestmark = pytest.mark.gpu
STRIP, ROWS = EXCEEDANCE_STRIP, EXCEEDANCE_ROWS
LAYOUTS = ["i32", "u24", "u16"]
SHAPES = [(1, 1, 1), (63, 1, 2), (64, 2, 3), (65, 3, 5), (130, 3, 17), (1000, 5, 33)]
LARGEST = (1000, 33, 70)
assert STRIP == 8 and ROWS == 8 and EXCEEDANCE_NA == NA and EXCEEDANCE_MAX_NORMALS == MAX_NORMALS


def ex_records(P, n, seed, max_count=65534, extras=0):
    """int32 [n, P + extras, 8]: depths per strand from a short menu around the cut-off of 100 (0, 99, 100, 101, 200, 1000, 2000) and
    alternative counts that are round fractions of them (0, 1 %, 3 %, 5 %, 50 %), so that x_s D_t == x_t D_s happens all the time, with
    one read more or less on a third of them; a tenth of the records uniformly random; a tenth absent"""
    rng = np.random.default_rng(seed)
    R = P + extras
    recs = np.zeros((n, R, 8), np.int64)
    major = rng.integers(0, 4, R)
    for st in range(2):
        d = rng.choice([0, 99, 100, 101, 200, 1000, 2000], (n, R), p=[0.04, 0.06, 0.1, 0.1, 0.2, 0.25, 0.25])
        k = (d[:, :, None] * rng.choice([0.0, 0.01, 0.03, 0.05, 0.5], (n, R, 4), p=[0.3, 0.25, 0.2, 0.15, 0.1])).astype(np.int64)
        k += rng.choice([-1, 0, 1], (n, R, 4), p=[1 / 6, 2 / 3, 1 / 6])
        k = np.clip(k, 0, None)
        np.put_along_axis(k, np.broadcast_to(major[None, :, None], (n, R, 1)), 0, axis=2)
        k[k.sum(-1) > d] = 0
        np.put_along_axis(k, np.broadcast_to(major[None, :, None], (n, R, 1)), (d - k.sum(-1))[:, :, None], axis=2)
        recs[:, :, 4 * st:4 * st + 4] = k
    kind = rng.random((n, R))
    wild = kind < 0.1
    recs[wild] = rng.integers(0, max_count + 1, (int(wild.sum()), 8))
    recs = recs.clip(0, max_count)
    recs[kind > 0.9] = [ABSENT, 0, 0, 0, 0, 0, 0, 0]
    recs = recs.astype(np.int32)
    recs.setflags(write=False)
    return recs


def ref_codes(P, seed):
    ref = np.random.default_rng(500 + seed).choice([0, 1, 2, 3, 4, 255], P, p=[0.24, 0.24, 0.24, 0.24, 0.02, 0.02]).astype(np.uint8)
    ref.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def _case(P, n_t, n_n, **kw):
    t, n, ref = ex_records(P, n_t, 31 * P + n_t), ex_records(P, n_n, 37 * P + n_n + 1), ref_codes(P, P + n_n)
    e, g = exceedance(t, n, ref, **kw)
    e.setflags(write=False)
    g.setflags(write=False)
    return t, n, ref, e, g


def u16(t):
    return t.cpu().numpy().view(np.uint16)


def _run(ctx, t, n, lt, ln, P, ref, **kw):
    rt, rn = ctx.records(_pack(ctx, t, lt), lt, t.shape[0]), ctx.records(_pack(ctx, n, ln), ln, n.shape[0])
    e, g = ctx.exceedance(rt, rn, P, ref, **kw)
    e, g = u16(e), u16(g)
    assert e.shape == (t.shape[0], P) and g.shape == (t.shape[0], P, 4, 2)
    return e, g


def _same(got, exp):
    return np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1])


@pytest.mark.parametrize("ln", LAYOUTS)
@pytest.mark.parametrize("lt", LAYOUTS)
@pytest.mark.parametrize("P,n_t,n_n", SHAPES)
def test_counts_equal_the_model(ctx, P, n_t, n_n, lt, ln):
    t, n, ref, e, g = _case(P, n_t, n_n)
    if P >= 1000:  # the data meet every clause: NA and counted cells, ties, cells every normal reaches and cells none does
        ev, all_of_them = g != NA, np.broadcast_to(e[:, :, None, None], g.shape)
        assert 0.3 < ev.mean() < 0.8 and (e < n_n).any() and (g[ev] == 0).any() and (g[ev] == all_of_them[ev]).any() and (g[ev] < all_of_them[ev]).any()
    assert _same(_run(ctx, t, n, lt, ln, P, ref), (e, g))


def test_the_largest_shape_with_a_mixed_pair(ctx):
    P, n_t, n_n = LARGEST
    t, n, ref, e, g = _case(P, n_t, n_n)
    assert (e > 50).any()
    assert _same(_run(ctx, t, n, "u16", "i32", P, ref), (e, g))


@pytest.mark.parametrize("n_n", [STRIP - 1, STRIP, STRIP + 1, 2 * STRIP + 1])
@pytest.mark.parametrize("lt,ln", [("u16", "u16"), ("i32", "u24")])
def test_normals_around_the_strip(ctx, n_n, lt, ln):
    t, n, ref, e, g = _case(130, 3, n_n)
    assert _same(_run(ctx, t, n, lt, ln, 130, ref), (e, g))


@pytest.mark.parametrize("n_t", [ROWS - 1, ROWS, ROWS + 1])
@pytest.mark.parametrize("lt,ln", [("u16", "u16"), ("u24", "i32")])
def test_tumour_rows_around_the_row_group(ctx, n_t, lt, ln):
    t, n, ref, e, g = _case(130, n_t, 5)
    assert _same(_run(ctx, t, n, lt, ln, 130, ref), (e, g))


@pytest.mark.parametrize("ncut,ccut", [(0, 0), (1, 101), (99, 100), (101, 99), (2000, 2001), (30000, 0)])
def test_the_cut_offs(ctx, ncut, ccut):
    t, n, ref, _, _ = _case(1000, 5, 33)
    exp = exceedance(t, n, ref, normal_cutoff=ncut, calling_cutoff=ccut)
    assert _same(_run(ctx, t, n, "u16", "u24", 1000, ref, normal_cutoff=ncut, calling_cutoff=ccut), exp)


@pytest.mark.parametrize("lt,ln", [("i32", "u16"), ("u24", "u24"), ("u16", "i32")])
def test_a_padded_row_stride(ctx, lt, ln):
    P, n_t, n_n, pad_t, pad_n = 65, ROWS + 2, STRIP + 3, 7, 3
    t, n, ref = ex_records(P + pad_t, n_t, 21), ex_records(P + pad_n, n_n, 22), ref_codes(P, 23)  # the pads hold records too
    rt = ctx.records(_pack(ctx, t, lt), lt, n_t, row_stride=P + pad_t)
    rn = ctx.records(_pack(ctx, n, ln), ln, n_n, row_stride=P + pad_n)
    e, g = ctx.exceedance(rt, rn, P, ref)
    assert _same((u16(e), u16(g)), exceedance(t[:, :P], n[:, :P], ref))


@pytest.mark.parametrize("layout", ["i32", "u24"])
def test_extras_and_an_rd_plane_do_not_matter(ctx, layout):
    P, n_t, n_n, E = 130, 5, 11, 9
    t, n, ref = ex_records(P, n_t, 77, extras=E), ex_records(P, n_n, 78, extras=E), ref_codes(P, 79)
    rng = np.random.default_rng(4)
    dup_off = np.concatenate([[0], np.cumsum(np.isin(np.arange(P), rng.choice(P, E, replace=False)))]).astype(np.uint32)
    ext_pos = np.repeat(np.arange(P), np.diff(dup_off.astype(np.int64))).astype(np.uint32)

    def full(r, k):
        rd = np.where(rng.random((k, P + E)) < 0.3, 12345, ABSENT).astype(np.int32)
        return ctx.records(_pack(ctx, r, layout), layout, k, E=E, dup_off=_t(dup_off), ext_pos=_t(ext_pos), rd=_t(rd[:, :P]), rd_ext=_t(rd[:, P:]))

    a = ctx.exceedance(full(t, n_t), full(n, n_n), P, ref)
    b = ctx.exceedance(ctx.records(_pack(ctx, t[:, :P], layout), layout, n_t), ctx.records(_pack(ctx, n[:, :P], layout), layout, n_n), P, ref)
    exp = exceedance(t[:, :P], n[:, :P], ref)
    assert _same((u16(a[0]), u16(a[1])), exp) and _same((u16(b[0]), u16(b[1])), exp) and (exp[1] != NA).any()


def test_i32_fields_of_two_to_the_thirty_and_beyond(ctx):
    P, n_t, n_n = 700, ROWS + 1, STRIP + 3
    big, top = 1 << 30, (1 << 31) - 1
    menu = np.array([[big, 0, 0, 1 << 24, big, 0, 0, 1 << 24], [top, top // 100, top // 100, top // 100, top, 0, 0, 0], [top, 0, 0, 0, top, 0, 0, 0],
                     [top, top, top, top, top, top, top, top], [top, top, top, top - 1, top, top - 1, top, top], [top, top - 1, top, top - 1, top, top, top - 1, top],
                     [big, big, big, big, big, big, big, big], [99, 0, 0, 0, top, top, 0, 0], [3, 1, 0, 0, 3, 1, 0, 0], [3, 0, 5, top, 0, 0, 0, 99],
                     [ABSENT, top, 0, 0, top, 0, 0, 0]], np.int64).astype(np.int32)
    rng = np.random.default_rng(30)
    t, n = menu[rng.integers(0, len(menu), (n_t, P))], menu[rng.integers(0, len(menu), (n_n, P))]
    ref = ref_codes(P, 31)
    for cut in (100, 0):
        exp = exceedance(t, n, ref, normal_cutoff=cut, calling_cutoff=cut)
        assert (exp[1] != NA).any() and (exp[1][exp[1] != NA] > 0).any()
        assert _same(_run(ctx, t, n, "i32", "i32", P, ref, normal_cutoff=cut, calling_cutoff=cut), exp)
    # a 16-bit side against the widest int32 side: both mixed paths multiply a count by a 33-bit depth
    s = ex_records(P, n_t, 32)
    assert _same(_run(ctx, s, n, "u16", "i32", P, ref), exceedance(s, n, ref))
    assert _same(_run(ctx, t, ex_records(P, n_n, 33), "i32", "u24", P, ref), exceedance(t, ex_records(P, n_n, 33), ref))


@pytest.mark.parametrize("cuts", [(0, 33), (0, 8, 33), (0, 1, 9, 17, 18, 33)])
@pytest.mark.parametrize("lt,ln", [("u16", "u16"), ("i32", "u24")])
def test_normals_in_chunks_into_the_same_outputs(ctx, cuts, lt, ln):
    import torch

    P, n_t, n_n = 1000, 5, 33
    t, n, ref, e1, g1 = _case(P, n_t, n_n, first_t=40, first_n=10)
    rt, d_ref = ctx.records(_pack(ctx, t, lt), lt, n_t), _t(ref)
    elig = torch.full((n_t, P), -1, dtype=torch.int16, device=ctx.device)
    ge = torch.full((n_t, P, 4, 2), 0x5A5A, dtype=torch.int16, device=ctx.device)
    for k, (lo, hi) in enumerate(zip(cuts[:-1], cuts[1:])):
        out = ctx.exceedance(rt, ctx.records(_pack(ctx, n[lo:hi], ln), ln, hi - lo), P, d_ref, first_t=40, first_n=10 + lo, accumulate=k > 0, elig=elig, ge=ge)
        assert out[0].data_ptr() == elig.data_ptr() and out[1].data_ptr() == ge.data_ptr()
        if k == 0:  # what is NA after the first chunk is NA at the end, and nothing else is
            na = u16(ge) == NA
    assert _same((u16(elig), u16(ge)), (e1, g1))
    assert np.array_equal(u16(ge) == NA, na) and na.any() and not na.all()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_skip_same_index_with_the_same_chunk_on_both_sides(ctx, layout):
    P, n = 130, 2 * STRIP + 3
    recs, ref = ex_records(P, n, 9), ref_codes(P, 9)
    rec = ctx.records(_pack(ctx, recs, layout), layout, n)
    for first_t, first_n, skip in ((0, 0, True), (5, 5, True), (3, 5, True), (9, 5, True), (5, 5, False), (100, 5, True)):
        exp = exceedance(recs, recs, ref, first_t=first_t, first_n=first_n, skip_same_index=skip)
        e, g = ctx.exceedance(rec, rec, P, ref, first_t=first_t, first_n=first_n, skip_same_index=skip)
        assert _same((u16(e), u16(g)), exp), (first_t, first_n, skip)
    a = exceedance(recs, recs, ref, skip_same_index=True)
    b = exceedance(recs, recs, ref, skip_same_index=False)
    assert not np.array_equal(a[0], b[0]) and (b[0].astype(int) - a[0] <= 1).all()


def test_two_runs_are_bit_identical(ctx):
    P, n_t, n_n = LARGEST
    t, n, ref, e, g = _case(P, n_t, n_n)
    rt, rn = ctx.records(_pack(ctx, t, "u24"), "u24", n_t), ctx.records(_pack(ctx, n, "u16"), "u16", n_n)
    one = [u16(x).tobytes() for x in ctx.exceedance(rt, rn, P, ref)]
    two = [u16(x).tobytes() for x in ctx.exceedance(rt, rn, P, ref)]
    assert one == two == [e.tobytes(), g.tobytes()]


def test_planted_cohort_end_to_end(ctx):
    c, r = planted(), planted_results()
    P, recs = c["P"], c["recs"]
    cut = dict(normal_cutoff=DEFAULTS["coverage_cutoff"], calling_cutoff=DEFAULTS["calling_cutoff"])
    rn = ctx.records(_pack(ctx, recs[:N_NORMALS], "u16"), "u16", N_NORMALS)
    rt = ctx.records(_pack(ctx, recs[N_NORMALS:], "u16"), "u16", len(recs) - N_NORMALS)
    e, g = (u16(x) for x in ctx.exceedance(rt, rn, P, c["ref_code"], first_t=N_NORMALS, **cut))
    assert np.array_equal(e, r["elig"]) and np.array_equal(g, r["ge"])
    cand = candidates(recs[N_NORMALS:], e, g, **CAND)
    assert np.array_equal(cand, r["cand"]) and all(cand[1, p, y] for p, y in c["variants"]) and not any(cand[2, p, y] for p, y in c["hets"])
    e, g = (u16(x) for x in ctx.exceedance(rn, rn, P, c["ref_code"], skip_same_index=True, **cut))
    assert np.array_equal(e, r["self_elig"]) and np.array_equal(g, r["self_ge"])
