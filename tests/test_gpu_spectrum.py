"""Context.spectrum (ampli_spectrum.hip) against the definition (tests/spectrum_model.py), exactly: np.array_equal on the int64 sums.

Shapes: every record layout at (P, n) = (1, 1), (63, 1), (64, 2), (65, 3), (130, strip - 1), (1000, strip + 1) and (1000, 33) -- one
tile, a partial tile, a tile and one lane, several tiles per wave, a partial strip, several strips; a shape the launcher's rule cuts
into several position segments (the atomic form) and one with many rows it leaves whole (the store form), told apart by
ampli_last_spectrum_segments.  Class arrays: every position in one class (every lane on one bin), C = 1 and C = 128, all 255, values in
[C, 255), a class without a position.  A padded row stride; absent records; extras and an RD plane without effect; int32 fields of
2^30 and 2^31 - 1 with sums beyond 2^40; chunks into the rows of one matrix; bit-identical repeats; the cut-off and max_alt_pm at their
edges; the planted cohort end to end."""
import functools

import numpy as np
import pytest

from amplisolve_amd.api import SPEC_SUMS, SPECTRUM_MAX_CLASSES, SPECTRUM_STRIP
from tests.spectrum_cohorts import N_NORMALS, planted, planted_results
from tests.spectrum_model import ABSENT, CLASSES, DEFAULTS, class_sums, enters, fold, score
from tests.test_gpu_loo import _pack
from tests.test_gpu_parity import _t

pytestmark = pytest.mark.gpu
STRIP = SPECTRUM_STRIP
SHAPES = [(1, 1), (63, 1), (64, 2), (65, 3), (130, STRIP - 1), (1000, STRIP + 1), (1000, 33)]
assert STRIP == 4 and SPEC_SUMS == 9 and SPECTRUM_MAX_CLASSES == 128


def spec_records(P, n, seed, max_count=65534, extras=0):
    """int32 [n, P + extras, 8] and ref_code uint8 [P]: half of the records background (deep on the reference base, alternatives of a
    few per mille), the others at the gate's edges -- an alternative exactly at 30 per mille of the depth and one read above, a strand
    at the cut-off and one read below, no reads at all, a heterozygous position, an absent record -- or uniformly random"""
    rng = np.random.default_rng(seed)
    R = P + extras
    ref = rng.choice([0, 1, 2, 3, 4, 255], P, p=[0.24, 0.24, 0.24, 0.24, 0.02, 0.02]).astype(np.uint8)
    r = np.concatenate([np.where(ref <= 3, ref, 0), rng.integers(0, 4, extras)]).astype(np.int64)
    kind = rng.choice(8, (n, R), p=[0.5, 0.1, 0.1, 0.08, 0.05, 0.05, 0.05, 0.07])
    recs = np.zeros((n, R, 8), np.int64)
    deep = min(max_count // 2, 4000)
    depth = rng.integers(150, deep, (n, R, 2))
    depth[kind == 3] = rng.choice([99, 100, 101], (int((kind == 3).sum()), 2))
    for st in range(2):
        alts = rng.poisson(depth[:, :, st, None] * 2e-3, (n, R, 4))
        alts[kind == 6] = (depth[:, :, st][kind == 6] * 0.45).astype(np.int64)[:, None] * (np.arange(4) == 1)
        np.put_along_axis(alts, np.broadcast_to(r[None, :, None], (n, R, 1)), 0, axis=2)
        recs[:, :, 4 * st:4 * st + 4] = alts
        own = depth[:, :, st] - alts.sum(-1)
        np.put_along_axis(recs[:, :, 4 * st:4 * st + 4], np.broadcast_to(r[None, :, None], (n, R, 1)), own[:, :, None], axis=2)
    # kinds 1 and 2: d a multiple of 1000 or not; one alternative (on the forward strand) at floor(30 d / 1000), or one above
    for k, add in ((1, 0), (2, 1)):
        m = kind == k
        d = recs[m].sum(-1)
        y = (r[None, :] + 1 + rng.integers(0, 3, (n, R))) % 4
        rows = recs[m]
        rows[np.arange(len(rows)), np.broadcast_to(r[None, :], (n, R))[m]] += rows[np.arange(len(rows)), y[m]] + rows[np.arange(len(rows)), 4 + y[m]]
        rows[np.arange(len(rows)), 4 + y[m]] = 0
        rows[np.arange(len(rows)), y[m]] = 0
        lim = 30 * d // 1000 + add
        rows[np.arange(len(rows)), np.broadcast_to(r[None, :], (n, R))[m]] -= lim
        rows[np.arange(len(rows)), y[m]] = lim
        recs[m] = rows
    recs[kind == 4] = 0
    recs[kind == 7] = rng.integers(0, max_count + 1, (int((kind == 7).sum()), 8))
    recs = recs.clip(0, max_count)
    recs[kind == 5] = [ABSENT, 0, 0, 0, 0, 0, 0, 0]
    recs = recs.astype(np.int32)
    recs.setflags(write=False)
    ref.setflags(write=False)
    return recs, ref


def classes(P, C, seed, skip=0.05):
    """uint8 [P]: uniform over [0, C), a share `skip` of 255"""
    rng = np.random.default_rng(1000 + seed)
    cls = rng.integers(0, C, P).astype(np.uint8)
    cls[rng.random(P) < skip] = 255
    cls.setflags(write=False)
    return cls


@functools.lru_cache(maxsize=None)
def _case(P, n, C=CLASSES):
    recs, ref = spec_records(P, n, 17 * P + n + 2)
    cls = classes(P, C, P + n)
    exp = class_sums(recs, ref, cls, C)
    exp.setflags(write=False)
    return recs, ref, cls, exp


def _run(ctx, recs, layout, P, ref, cls, C, **kw):
    n = recs.shape[0]
    got = ctx.spectrum(ctx.records(_pack(ctx, recs, layout), layout, n), P, ref, cls, C, **kw).cpu().numpy()
    assert got.shape == (n, C, 9) and got.dtype == np.int64
    return got


@pytest.mark.parametrize("layout", ["i32", "u24", "u16"])
@pytest.mark.parametrize("P,n", SHAPES)
def test_sums_equal_the_model(ctx, layout, P, n):
    recs, ref, cls, exp = _case(P, n)
    if P * n >= 5000:
        e = enters(recs, ref[None, :], cls[None, :], CLASSES)
        assert 0.3 < e.mean() < 0.8 and (recs[:, :, 0] == ABSENT).any() and (exp[:, :, 0] > 0).any(0).sum() >= 60
    assert np.array_equal(_run(ctx, recs, layout, P, ref, cls, CLASSES), exp)
    assert ctx.last_spectrum_segments() == 1


@pytest.mark.parametrize("layout,n,P", [("u16", 1, 70000), ("u24", STRIP + 1, 40000), ("i32", 2, 70001)])
def test_several_segments_add_into_the_cleared_matrix(ctx, layout, n, P):
    recs, ref, cls, exp = _case(P, n)
    assert (exp[:, :, 0] > 0).all()
    assert np.array_equal(_run(ctx, recs, layout, P, ref, cls, CLASSES), exp)
    assert ctx.last_spectrum_segments() > 1


def test_many_rows_stay_one_segment(ctx):
    P, n = 130, 2100
    recs, ref, cls, exp = _case(P, n)
    assert np.array_equal(_run(ctx, recs, "u16", P, ref, cls, CLASSES), exp)
    assert ctx.last_spectrum_segments() == 1


def test_class_arrays(ctx):
    P, n = 1000, STRIP + 1
    recs, ref, _, _ = _case(P, n)
    one = np.full(P, 5, np.uint8)                                   # every lane on one bin
    got = _run(ctx, recs, "u16", P, ref, one, CLASSES)
    assert np.array_equal(got, class_sums(recs, ref, one, CLASSES)) and got[:, 5, 0].min() > 300 and not got[:, :5].any() and not got[:, 6:].any()
    zero = np.zeros(P, np.uint8)
    assert np.array_equal(_run(ctx, recs, "u24", P, ref, zero, 1), class_sums(recs, ref, zero, 1))  # C == 1
    assert not _run(ctx, recs, "u24", P, ref, one, 1).any()       # class 5 is not below C == 1
    wide = classes(P, 128, 3)
    exp = class_sums(recs, ref, wide, 128)
    assert (exp[:, 127, 0] > 0).any() and np.array_equal(_run(ctx, recs, "i32", P, ref, wide, 128), exp)  # C == 128
    assert not _run(ctx, recs, "u16", P, ref, np.full(P, 255, np.uint8), CLASSES).any()               # all skipped
    high = np.random.default_rng(5).integers(CLASSES, 255, P).astype(np.uint8)                           # values in [C, 255)
    assert not _run(ctx, recs, "u16", P, ref, high, CLASSES).any()
    mixed = np.where(np.arange(P) % 3 == 0, high, wide)                                                  # ... among valid ones
    assert np.array_equal(_run(ctx, recs, "u16", P, ref, mixed, 100), class_sums(recs, ref, mixed, 100))
    holes = np.where(wide == 9, 10, wide)                                                                # a class no position has
    got = _run(ctx, recs, "u16", P, ref, holes, 128)
    assert np.array_equal(got, class_sums(recs, ref, holes, 128)) and not got[:, 9].any()
    assert not _run(ctx, recs, "u16", P, np.full(P, 255, np.uint8), wide, 128).any()                     # no reference base anywhere


@pytest.mark.parametrize("cov", [0, 1, 99, 100, 101, 30000])
def test_the_cut_off(ctx, cov):
    recs, ref, cls, _ = _case(1000, STRIP + 1)
    assert np.array_equal(_run(ctx, recs, "u16", 1000, ref, cls, CLASSES, cov=cov), class_sums(recs, ref, cls, CLASSES, cov))


@pytest.mark.parametrize("pm", [0, 1, 15, 29, 30, 31, 1000])
def test_max_alt_pm(ctx, pm):
    recs, ref, cls, _ = _case(1000, STRIP + 1)
    exp = class_sums(recs, ref, cls, CLASSES, 100, pm)
    assert np.array_equal(_run(ctx, recs, "u24", 1000, ref, cls, CLASSES, max_alt_pm=pm), exp)
    if pm in (29, 31):  # the planted edges move with it
        assert not np.array_equal(exp, class_sums(recs, ref, cls, CLASSES, 100, 30))


def test_no_reads_and_no_cut_off(ctx):
    """d == 0 passes the gate's last clause: with a cut-off of zero an empty record is a site"""
    P, n = 130, 2
    recs = np.zeros((n, P, 8), np.int32)
    recs[1, ::2] = [ABSENT, 0, 0, 0, 0, 0, 0, 0]
    ref, cls = np.zeros(P, np.uint8), np.full(P, 3, np.uint8)
    got = _run(ctx, recs, "u16", P, ref, cls, 4, cov=0)
    assert np.array_equal(got, class_sums(recs, ref, cls, 4, 0)) and got[:, 3, 0].tolist() == [130, 65] and got.sum() == 195
    assert not _run(ctx, recs, "u16", P, ref, cls, 4, cov=1).any()


@pytest.mark.parametrize("layout", ["i32", "u24", "u16"])
def test_a_padded_row_stride(ctx, layout):
    P, n, pad = 65, STRIP + 2, 7
    recs, _ = spec_records(P + pad, n, 21)  # the pad holds records too: they must not be read in place of the next row's
    _, ref = spec_records(P, 1, 22)
    cls = classes(P, CLASSES, 23)
    got = ctx.spectrum(ctx.records(_pack(ctx, recs, layout), layout, n, row_stride=P + pad), P, ref, cls, CLASSES).cpu().numpy()
    assert np.array_equal(got, class_sums(recs[:, :P], ref, cls, CLASSES))


@pytest.mark.parametrize("layout", ["i32", "u24"])
def test_extras_and_an_rd_plane_do_not_matter(ctx, layout):
    P, n, E = 130, 7, 9
    recs, ref = spec_records(P, n, 77, extras=E)
    cls = classes(P, CLASSES, 78)
    rng = np.random.default_rng(4)
    dup_off = np.concatenate([[0], np.cumsum(np.isin(np.arange(P), rng.choice(P, E, replace=False)))]).astype(np.uint32)
    ext_pos = np.repeat(np.arange(P), np.diff(dup_off.astype(np.int64))).astype(np.uint32)
    rd = np.where(rng.random((n, P + E)) < 0.3, 12345, ABSENT).astype(np.int32)
    full = ctx.records(_pack(ctx, recs, layout), layout, n, E=E, dup_off=_t(dup_off), ext_pos=_t(ext_pos), rd=_t(rd[:, :P]), rd_ext=_t(rd[:, P:]))
    plain = ctx.records(_pack(ctx, recs[:, :P], layout), layout, n)
    a, b = ctx.spectrum(full, P, ref, cls, CLASSES).cpu().numpy(), ctx.spectrum(plain, P, ref, cls, CLASSES).cpu().numpy()
    assert np.array_equal(a, b) and np.array_equal(a, class_sums(recs[:, :P], ref, cls, CLASSES)) and a.any()


def test_i32_fields_of_two_to_the_thirty_and_beyond(ctx):
    P, n = 6000, STRIP + 5
    big, top = 1 << 30, (1 << 31) - 1
    menu = np.array([[big, 0, 0, 1 << 24, big, 0, 0, 1 << 24], [top, top // 100, top // 100, top // 100, top, 0, 0, 0], [top, 0, 0, 0, top, 0, 0, 0],
                     [top, top, top, top, top, top, top, top], [99, 0, 0, 0, top, top, 0, 0], [3, 0, 5, top, 0, 0, 0, 99], [ABSENT, top, 0, 0, top, 0, 0, 0]],
                    np.int64).astype(np.int32)
    recs = menu[np.random.default_rng(30).integers(0, len(menu), (n, P))]
    ref, cls = np.zeros(P, np.uint8), classes(P, 2, 31, skip=0.0)
    exp = class_sums(recs, ref, cls, 2)
    assert (exp[:, :, [1, 5]] > 1 << 40).all() and (exp[:, :, 0] > 50).all() and (exp[:, :, 2] > 0).all()
    assert np.array_equal(_run(ctx, recs, "i32", P, ref, cls, 2), exp)
    assert np.array_equal(_run(ctx, recs, "i32", P, ref, cls, 2, max_alt_pm=1000, cov=0), class_sums(recs, ref, cls, 2, 0, 1000))


@pytest.mark.parametrize("layout", ["i32", "u24", "u16"])
def test_chunks_into_the_rows_of_one_matrix(ctx, layout):
    import torch

    P, n, cuts = 1000, 33, (0, 3, 4, 9, 24, 33)
    recs, ref, cls, exp = _case(P, n)
    d_ref, d_cls = _t(ref), _t(cls)
    buf = torch.full((n, CLASSES, 9), -1, dtype=torch.int64, device=ctx.device)
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        out = ctx.spectrum(ctx.records(_pack(ctx, recs[lo:hi], layout), layout, hi - lo), P, d_ref, d_cls, CLASSES, out=buf[lo:hi])
        assert out.data_ptr() == buf[lo:hi].data_ptr()
    assert np.array_equal(buf.cpu().numpy(), exp)


def test_two_runs_are_bit_identical(ctx):
    for P, n, segments in ((1000, 33, 1), (70000, 1, 2)):
        recs, ref, cls, exp = _case(P, n)
        rec = ctx.records(_pack(ctx, recs, "u24"), "u24", n)
        one = ctx.spectrum(rec, P, ref, cls, CLASSES).cpu().numpy().tobytes()
        two = ctx.spectrum(rec, P, ref, cls, CLASSES).cpu().numpy().tobytes()
        assert one == two == exp.tobytes() and (ctx.last_spectrum_segments() > 1) == (segments > 1)


def test_planted_cohort_end_to_end(ctx):
    c, r = planted(), planted_results()
    n, P = c["recs"].shape[0], c["P"]
    sums = ctx.spectrum(ctx.records(_pack(ctx, c["recs"], "u16"), "u16", n), P, c["ref_code"], c["cls"], CLASSES, cov=DEFAULTS["coverage_cutoff"],
                        max_alt_pm=DEFAULTS["max_alt_pm"]).cpu().numpy()
    assert np.array_equal(sums, r["sums"])
    sc = score(fold(sums), N_NORMALS, **{k: DEFAULTS[k] for k in ("min_sites", "min_normals", "excess_ratio", "z_cutoff", "asym_delta")})
    assert np.array_equal(sc["flag"], r["score"]["flag"]) and set(sc["flag"].ravel().tolist()) == {0, 1, 3, 4}
