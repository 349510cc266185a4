"""Context.genotype_planes (genotype_planes_kernel) and Context.concordance (concordance_pairs_kernel) against the definition
(tests/concordance_model.py), exactly: the planes word for word on every record layout, on shapes with one full word, one bit in a
second word and a partial word only, on chunked cohorts written into the rows of one buffer, with extra occurrences and an RD plane
(which must not matter) and with int32 counts up to 2^30 per field; the pair counts on tiles that are full, partial and single rows and
on word counts below, at and beyond one slab of the kernel (8 words; P = 4200 is 66 words: eight slabs and a remainder); the
same-pointer form against the two-pointer form; the planted cohort's relations; bit-identical repeats."""
import functools

import numpy as np
import pytest

from tests.concordance_cohorts import boundary_grid, planted, planted_counts, records
from tests.concordance_model import ABSENT, H, V, classify, pack_planes, pair_counts, planes, relations, words
from tests.test_gpu_loo import _pack
from tests.test_gpu_parity import _t

pytestmark = pytest.mark.gpu


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _dev(pl):
    return _t(pl.view(np.int64))


@functools.lru_cache(maxsize=None)
def _pool(P):
    """130 samples' plane bits and planes at P positions, from the model, shared by the pair tests"""
    bits = classify(records(P, 130, 1000 + P))
    pl = pack_planes(bits, P)
    bits.setflags(write=False)
    pl.setflags(write=False)
    return bits, pl


@pytest.mark.parametrize("layout", ["i32", "u24", "u16"])
@pytest.mark.parametrize("P,n", [(64, 1), (65, 2), (77, 1), (130, 7), (1000, 64)])
def test_planes_equal_the_model(ctx, layout, P, n):
    recs = records(P, n, P + n)  # counts <= 65534: one cohort for every layout; the boundary grid and absent records planted
    exp = planes(recs, P)
    if P * n >= 500:
        assert (exp[:, 0] != 0).any() and (exp[:, 5] != 0).any() and (recs[:, :, 0] == ABSENT).any()
    got = _u64(ctx.genotype_planes(ctx.records(_pack(ctx, recs, layout), layout, n), P))
    assert got.shape == (n, 6, words(P)) and np.array_equal(got, exp)


@pytest.mark.parametrize("layout", ["i32", "u24", "u16"])
@pytest.mark.parametrize("P,n,cuts", [(130, 7, (0, 3, 7)), (1000, 64, (0, 20, 41, 64))])
def test_chunks_into_the_rows_of_one_buffer(ctx, layout, P, n, cuts):
    import torch

    recs = records(P, n, P + n)
    buf = torch.full((n, 6, words(P)), -1, dtype=torch.int64, device=ctx.device)
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        out = ctx.genotype_planes(ctx.records(_pack(ctx, recs[lo:hi], layout), layout, hi - lo), P, out=buf[lo:hi])
        assert out.data_ptr() == buf[lo:hi].data_ptr()
    assert np.array_equal(_u64(buf), planes(recs, P))


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
    a, b = _u64(ctx.genotype_planes(full, P)), _u64(ctx.genotype_planes(plain, P))
    assert np.array_equal(a, b) and np.array_equal(a, planes(recs, P))
    assert not np.array_equal(classify(recs[:, P:]), classify(recs[:, ext_pos]))  # the extras do differ from their primaries


def test_i32_deep_records_and_two_to_the_thirty_per_field(ctx):
    P, n = 300, 5
    recs = records(P, n, 21, max_count=None).copy()  # depths up to 2^26 and the whole grid: 2^30 per field, 2^31 - 1
    recs[0, 0] = 1 << 30
    recs[1, 1] = [1 << 30, 0, 0, 0, 1 << 30, 0, 0, 0]
    deep = np.where(recs[:, :, 0] == ABSENT, 0, recs.astype(np.int64).sum(-1))
    assert (deep >= 1 << 22).sum() >= 50 and (deep >= 1 << 33).any()
    exp = planes(recs, P)
    assert exp[0, 0, 0] & np.uint64(1) == 0 and exp[1, 0, 0] & np.uint64(2) == 2
    got = _u64(ctx.genotype_planes(ctx.records(_t(recs), "i32", n), P))
    assert np.array_equal(got, exp)


def test_other_parameters(ctx):
    P, n = 200, 3
    prm = dict(min_depth=30, absent_max_pm=50, het_min_pm=300, het_max_pm=300, hom_min_pm=950)
    recs = np.concatenate([boundary_grid(**prm), boundary_grid()])[:P * n].reshape(n, P, 8)
    recs = np.where(recs == ABSENT, ABSENT, np.minimum(recs, 65534)).astype(np.int32)
    got = _u64(ctx.genotype_planes(ctx.records(_pack(ctx, recs, "u24"), "u24", n), P, **prm))
    assert np.array_equal(got, planes(recs, P, **prm)) and not np.array_equal(got, planes(recs, P))


@pytest.mark.parametrize("P", [64, 65, 1000, 4200])
@pytest.mark.parametrize("n_a,n_b", [(1, 1), (2, 2), (7, 7), (5, 70), (70, 5), (33, 65), (130, 130)])
def test_pair_counts_equal_the_model(ctx, P, n_a, n_b):
    bits, pl = _pool(P)
    a, b = slice(0, n_a), slice(130 - n_b, 130)  # two different (overlapping) sets of rows
    got = ctx.concordance(_dev(pl[a]), _dev(pl[b]), P).cpu().numpy()
    exp = pair_counts(bits[a], bits[b])
    assert got.shape == (n_a, n_b, 5) and got.dtype == np.int32 and np.array_equal(got, exp)
    if P >= 1000:
        assert (exp[:, :, 0] > P // 20).all() and (exp[:, :, 1:] > 0).any(axis=(0, 1)).all()


@pytest.mark.parametrize("P,n", [(65, 1), (65, 33), (1000, 70), (4200, 130), (64, 129)])
def test_one_pointer_equals_two_pointers_and_is_symmetric(ctx, P, n):
    bits, pl = _pool(P)
    d = _dev(pl[:n])
    one = ctx.concordance(d, d, P).cpu().numpy()
    two = ctx.concordance(d, d.clone(), P).cpu().numpy()
    assert np.array_equal(one, two) and np.array_equal(one, pair_counts(bits[:n], bits[:n]))
    assert np.array_equal(one, one.transpose(1, 0, 2))  # all five counts, het_match too
    popc = lambda k: np.array([sum(bin(int(w)).count("1") for w in pl[s, k]) for s in range(n)])
    assert np.array_equal(np.diagonal(one[:, :, 0]), popc(0)) and np.array_equal(np.diagonal(one[:, :, 3]), popc(5))
    assert np.array_equal(np.diagonal(one[:, :, 1]), popc(0)) and np.array_equal(np.diagonal(one[:, :, 4]), popc(5)) and (np.diagonal(one[:, :, 2]) == 0).all()


def test_planted_cohort_and_repeats(ctx):
    recs, who = planted()
    n, P = recs.shape[0], recs.shape[1]
    runs = []
    for _ in range(2):
        pl = ctx.genotype_planes(ctx.records(_pack(ctx, recs, "u16"), "u16", n), P)
        runs.append((pl.cpu().numpy().tobytes(), ctx.concordance(pl, pl, P).cpu().numpy()))
    assert runs[0][0] == runs[1][0] and runs[0][1].tobytes() == runs[1][1].tobytes()
    counts = runs[0][1]
    assert np.array_equal(counts, planted_counts())
    rel = relations(counts, 20, 0.8)
    same = who[:, None] == who[None, :]
    assert np.array_equal(rel, relations(planted_counts(), 20, 0.8)) and (rel[same] == 1).all() and (rel[~same] == 2).all()
    assert np.array_equal(np.diagonal(counts[:, :, 0]), ((classify(recs) & V) != 0).sum(1)) and (np.diagonal(counts[:, :, 3]) == ((classify(recs) & H) != 0).sum(1)).all()
