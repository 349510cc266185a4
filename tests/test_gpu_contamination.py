"""Context.contamination (contamination_kernel) against the definition (tests/contamination_model.py), exactly (np.array_equal on
int64).  The planes are uploaded from the model, so the kernel is tested apart from the encoder -- but for the planted cohort, which
goes end to end.

Shapes (P, n, n_b) and what the launcher makes of them on the 256 compute units of an MI355X (ct_slices in ampli_contamination.hip:
waves = n * ceil(n_b / 64); want = min(16, ceil(32 * 256 / waves)) slices of at least 4 words, all equal but the last):
  (64, 1, 1)       1 word,   1 source tile (one live lane),               1 slice
  (65, 2, 2)       2 words (one bit in the second),                        1 slice of 2 words
  (77, 3, 65)      2 words (a partial word only), one lane of a 2nd tile,  1 slice
  (130, 7, 64)     3 words, an exactly full tile,                          1 slice of 3 words
  (1000, 64, 130)  16 words, 3 tiles, 192 waves -> want 16,                4 slices of 4 words, added with atomics
  (4200, 5, 70)    66 words, 2 tiles, 10 waves -> want 16, 5 words each,   14 slices: 13 of 5 words and a last one of 1
on every record layout; a chunked recipient set written into the rows of one matrix; extra occurrences and an RD plane (which must not
matter); int32 counts of 2^30 and 2^31 - 1 per field, sums beyond 2^40; a set against itself and against a disjoint set; bit-identical
repeats; the planted cohort's statuses."""
import functools

import numpy as np
import pytest

from tests.concordance_cohorts import records
from tests.concordance_model import ABSENT, H, V, classify, pack_planes, words
from tests.contamination_cohorts import planted, planted_sums
from tests.contamination_model import CLEAN, CONTAMINATED, UNDETERMINED, statuses, sums
from tests.test_gpu_loo import _pack
from tests.test_gpu_parity import _t

pytestmark = pytest.mark.gpu
SHAPES = [(64, 1, 1), (65, 2, 2), (77, 3, 65), (130, 7, 64), (1000, 64, 130), (4200, 5, 70)]


def _dev(pl):
    return _t(pl.view(np.int64))


@functools.lru_cache(maxsize=None)
def _sources(P):
    """130 sources' plane bits and planes at P positions, from the model"""
    bits = classify(records(P, 130, 1000 + P))
    pl = pack_planes(bits, P)
    bits.setflags(write=False)
    pl.setflags(write=False)
    return bits, pl


@functools.lru_cache(maxsize=None)
def _case(P, n, n_b):
    """recipients (counts <= 65534: one cohort for every layout), their bits and planes, the sources' bits and planes, the model's sums"""
    recs = records(P, n, P + n)
    bits_a = classify(recs)
    bits_b, pl_b = _sources(P)
    exp = sums(recs, bits_a, bits_b[:n_b])
    exp.setflags(write=False)
    return recs, bits_a, pack_planes(bits_a, P), bits_b[:n_b], pl_b[:n_b], exp


@pytest.mark.parametrize("layout", ["i32", "u24", "u16"])
@pytest.mark.parametrize("P,n,n_b", SHAPES)
def test_sums_equal_the_model(ctx, layout, P, n, n_b):
    recs, bits_a, pl_a, bits_b, pl_b, exp = _case(P, n, n_b)
    if P * n >= 5000:
        assert (exp > 0).any(axis=(0, 1)).all() and (recs[:, :, 0] == ABSENT).any()  # every one of the nine sums is exercised
    got = ctx.contamination(ctx.records(_pack(ctx, recs, layout), layout, n), P, _dev(pl_a), _dev(pl_b)).cpu().numpy()
    assert got.shape == (n, n_b, 9) and got.dtype == np.int64 and np.array_equal(got, exp)


@pytest.mark.parametrize("layout", ["i32", "u24", "u16"])
@pytest.mark.parametrize("P,n,n_b,cuts", [(130, 7, 64, (0, 3, 7)), (1000, 64, 130, (0, 20, 41, 64))])
def test_chunks_into_the_rows_of_one_matrix(ctx, layout, P, n, n_b, cuts):
    import torch

    recs, bits_a, pl_a, bits_b, pl_b, exp = _case(P, n, n_b)
    buf = torch.full((n, n_b, 9), -1, dtype=torch.int64, device=ctx.device)
    da, db = _dev(pl_a), _dev(pl_b)
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        out = ctx.contamination(ctx.records(_pack(ctx, recs[lo:hi], layout), layout, hi - lo), P, da[lo:hi], db, out=buf[lo:hi])
        assert out.data_ptr() == buf[lo:hi].data_ptr()
    assert np.array_equal(buf.cpu().numpy(), exp)


@pytest.mark.parametrize("layout", ["i32", "u24"])
def test_extras_and_an_rd_plane_do_not_matter(ctx, layout):
    P, n, n_b, E = 130, 7, 64, 9
    recs = records(P, n, 77, extras=E)
    rng = np.random.default_rng(4)
    dup_off = np.concatenate([[0], np.cumsum(np.isin(np.arange(P), rng.choice(P, E, replace=False)))]).astype(np.uint32)
    ext_pos = np.repeat(np.arange(P), np.diff(dup_off.astype(np.int64))).astype(np.uint32)
    rd = np.where(rng.random((n, P + E)) < 0.3, 12345, ABSENT).astype(np.int32)
    full = ctx.records(_pack(ctx, recs, layout), layout, n, E=E, dup_off=_t(dup_off), ext_pos=_t(ext_pos), rd=_t(rd[:, :P]), rd_ext=_t(rd[:, P:]))
    plain = ctx.records(_pack(ctx, recs[:, :P], layout), layout, n)
    bits_a = classify(recs[:, :P])
    bits_b, pl_b = _sources(P)
    da, db = _dev(pack_planes(bits_a, P)), _dev(pl_b[:n_b])
    a, b = ctx.contamination(full, P, da, db).cpu().numpy(), ctx.contamination(plain, P, da, db).cpu().numpy()
    assert np.array_equal(a, b) and np.array_equal(a, sums(recs[:, :P], bits_a, bits_b[:n_b]))


def test_i32_fields_of_two_to_the_thirty_and_beyond(ctx):
    P, n, n_b = 2000, 4, 70
    big, top = 1 << 30, (1 << 31) - 1
    menu = np.array([[big, 0, 0, 1 << 25, big, 0, 0, 1 << 25], [top, 1 << 27, 0, 0, top, 1 << 27, 0, 0], [0, top, top >> 5, 0, 0, top, 0, 7],
                     [1 << 24, 0, big, 1 << 24, 1 << 23, 0, big, 0], [3, 0, 5, top, 0, 0, 0, top], [top, top, 0, 0, top, top, 0, 0],
                     [ABSENT, top, 0, 0, top, 0, 0, 0]], np.int64).astype(np.int32)
    rng = np.random.default_rng(30)
    recs = menu[rng.integers(0, len(menu), (n, P))]
    bits_a = classify(recs)
    hom = ((bits_a & V) != 0) & ((bits_a & H) == 0)
    assert hom.mean() > 0.5 and ((bits_a & H) != 0).any()
    recs[0, :3] = menu[6]                      # absent records ...
    bits_a[0, :3] = classify(menu[:1])[0]      # ... under set V bits: they count as zeros
    bits_b, pl_b = _sources(P)
    exp = sums(recs, bits_a, bits_b[:n_b])
    assert exp.max() > 1 << 40 and (exp[:, :, [1, 2, 4, 5, 7, 8]].max(axis=(0, 1)) > 1 << 32).all()  # every count sum beyond 32 bits
    got = ctx.contamination(ctx.records(_t(recs), "i32", n), P, _dev(pack_planes(bits_a, P)), _dev(pl_b[:n_b])).cpu().numpy()
    assert np.array_equal(got, exp)


@pytest.mark.parametrize("P,n", [(65, 2), (1000, 70)])
def test_a_set_against_itself_and_against_a_disjoint_set(ctx, P, n):
    recs = records(P, 2 * n, 3000 + P)
    bits = classify(recs)
    d = _dev(pack_planes(bits, P))
    rec = ctx.records(_pack(ctx, recs[:n], "u16"), "u16", n)
    own = ctx.contamination(rec, P, d[:n], d[:n]).cpu().numpy()
    assert np.array_equal(own, sums(recs[:n], bits[:n], bits[:n]))
    assert (own[np.arange(n), np.arange(n), :6] == 0).all()  # a sample carries no base that it does not carry
    hom = ((bits[:n] & V) != 0) & ((bits[:n] & H) == 0)
    assert np.array_equal(own[np.arange(n), np.arange(n), 6], hom.sum(1))
    other = ctx.contamination(rec, P, d[:n], d[n:]).cpu().numpy()
    assert np.array_equal(other, sums(recs[:n], bits[:n], bits[n:]))
    whole = ctx.contamination(rec, P, d[:n], d).cpu().numpy()  # the sources include the recipients' own rows
    assert np.array_equal(whole[:, :n], own) and np.array_equal(whole[:, n:], other)


@pytest.mark.parametrize("P,n,n_b", [(1000, 64, 130), (4200, 5, 70), (130, 7, 64)])
def test_two_runs_are_bit_identical(ctx, P, n, n_b):
    recs, bits_a, pl_a, bits_b, pl_b, exp = _case(P, n, n_b)
    rec, da, db = ctx.records(_pack(ctx, recs, "u24"), "u24", n), _dev(pl_a), _dev(pl_b)
    one = ctx.contamination(rec, P, da, db).cpu().numpy().tobytes()
    two = ctx.contamination(rec, P, da, db).cpu().numpy().tobytes()
    assert one == two == exp.tobytes()


def test_planted_cohort_end_to_end(ctx):
    recs, who = planted()
    n, P = recs.shape[0], recs.shape[1]
    rec = ctx.records(_pack(ctx, recs, "u16"), "u16", n)
    pl = ctx.genotype_planes(rec, P)
    got = ctx.contamination(rec, P, pl, pl).cpu().numpy()
    assert np.array_equal(got, planted_sums())
    st = statuses(got, 20, 0.005)
    assert np.array_equal(st, statuses(planted_sums(), 20, 0.005))
    assert st[6, 1] == CONTAMINATED and st[9, 0] == CLEAN and st[11, 2] == CONTAMINATED and st[10, 3] == UNDETERMINED
    assert (st[:6] != CONTAMINATED).all() and (st[np.arange(n), np.arange(n)] == UNDETERMINED).all()
    assert words(P) == 10  # 12 waves -> want 16, 4 words each: three slices, the last of two words
