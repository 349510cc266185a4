"""Context.hetsite_reference, allelic_sites and allelic_regions (csrc/ampli_allelic.hip) against the definition
(tests/allelic_model.py).  Integers, codes, masks, signs and v are exact (np.array_equal); |q| is within the paired suite's
S_TOL = 1e-5 of the model, whose tail shares nothing with the kernels' arithmetic.

Shapes (P, n) and what the launchers make of them: (64, 1) one full tile, one row; (65, 2) one bit in a second tile; (77, 3) a partial
tile only, fewer rows than the reference kernel has waves; (130, 7) three tiles, rows that do not fill the waves' turns evenly;
(1000, 64) 16 tiles, every wave of the reference kernel with 16 rows, site runs of one row; (4200, 5) 66 tiles.  On every record
layout; the planes are uploaded from the model, so the kernels are tested apart from the encoder."""
import functools

import numpy as np
import pytest

from tests import allelic_cohorts as ac
from tests import allelic_model as am
from tests.concordance_cohorts import records
from tests.concordance_model import ABSENT, classify, pack_planes
from tests.test_gpu_loo import _pack
from tests.test_gpu_parity import _t

pytestmark = pytest.mark.gpu
SHAPES = [(64, 1), (65, 2), (77, 3), (130, 7), (1000, 64), (4200, 5)]
LAYOUTS = ["i32", "u24", "u16"]
S_TOL = 1e-5  # tests/test_gpu_paired.py


def _dev(pl):
    return _t(np.ascontiguousarray(pl).view(np.int64))


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def _case(P, n, deep=False):
    """records (counts <= 65534 unless deep: one cohort for every layout), their plane bits and planes, the model's reference of them, a
    germline assignment (own row, the row before, none) over a second plane set, and the model's site planes"""
    recs = ac.small(P, n, 100 * P + n, layout_max=None if deep else 65534, deep=deep)
    bits = classify(recs)
    ref = am.reference(recs, bits, P, 100)
    # a panel-wide reference: the chunk's own rows alone would leave CNT below min_normals nearly everywhere
    pool = ac.small(P, 12, 7 * P + 1, layout_max=65534)
    ref_all = am.reference(pool, classify(pool), P, 100, ref)
    row_g = np.arange(n, dtype=np.int32)
    if n >= 3:
        row_g[1::3] -= 1  # another row's germline: its het sites meet absent and shallow records
        row_g[2] = -1
    exp = am.sites(recs, P, bits, row_g, ref_all, 100, 3, True)
    return _frozen(recs, bits, pack_planes(bits, P), ref, ref_all, row_g) + _frozen(*exp)


def _check_sites(got, exp):
    q, km, v, code = (x.cpu().numpy() for x in got)
    eq, ekm, ev, ecode, _ = exp
    assert np.array_equal(code, ecode) and np.array_equal(km, ekm) and np.array_equal(v, ev)
    t = (code >> 3) >= am.TESTED_REF
    assert np.array_equal(q[~t], eq[~t]) and np.array_equal(np.sign(q), np.sign(eq)) and not np.signbit(q[q == 0]).any()
    err = np.abs(np.abs(q[t].astype(np.float64)) - np.abs(eq[t].astype(np.float64)))
    print("tested", int(t.sum()), "max |q| error", float(err.max()) if t.any() else 0.0)
    assert (err <= S_TOL).all()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("P,n", SHAPES)
def test_reference_adds_to_what_is_there(ctx, layout, P, n):
    recs, bits, pl, ref = _case(P, n)[:4]
    if P * n >= 5000:
        assert (ref[0] > 0).any(axis=1).all() and (recs[:, :, 0] == ABSENT).any()  # all six pairs are exercised
    rec = ctx.records(_pack(ctx, recs, layout), layout, n)
    got = ctx.hetsite_reference(rec, P, _dev(pl), 100).cpu().numpy()
    assert got.shape == (3, 6, P) and got.dtype == np.int64 and np.array_equal(got, ref)
    start = np.random.default_rng(P).integers(0, 1 << 40, (3, 6, P))
    got = ctx.hetsite_reference(rec, P, _dev(pl), 100, ref=_t(start.copy())).cpu().numpy()
    assert np.array_equal(got, start + ref)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("P,n", SHAPES)
def test_sites_equal_the_model(ctx, layout, P, n):
    c = _case(P, n)
    recs, bits, pl, ref, ref_all, row_g = c[:6]
    if P * n >= 5000:
        st = c[9] >> 3
        assert all((st == s).any() for s in (am.NOT_HET, am.ABSENT_REC, am.SHALLOW, am.TESTED_REF, am.TESTED_HALF if n < 12 else am.TESTED_REF))
    got = ctx.allelic_sites(ctx.records(_pack(ctx, recs, layout), layout, n), P, _dev(pl), _t(row_g), _t(ref_all), 100, 3, True)
    _check_sites(got, c[6:])


@pytest.mark.parametrize("layout", ["i32", "u16"])
def test_chunked_rows_into_one_buffer(ctx, layout):
    import torch

    P, n, cuts = 1000, 64, (0, 20, 41, 64)
    c = _case(P, n)
    recs, bits, pl, ref, ref_all, row_g = c[:6]
    d = ctx.device
    q, km = torch.full((n, P), 7.0, dtype=torch.float32, device=d), torch.full((n, P, 2), -1, dtype=torch.int32, device=d)
    v, code = torch.full((n, P), -1.0, dtype=torch.float64, device=d), torch.full((n, P), 255, dtype=torch.uint8, device=d)
    acc = torch.zeros((3, 6, P), dtype=torch.int64, device=d)
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        rec = ctx.records(_pack(ctx, recs[lo:hi], layout), layout, hi - lo)
        ctx.hetsite_reference(rec, P, _dev(pl[lo:hi]), 100, ref=acc)
        ctx.allelic_sites(rec, P, _dev(pl), _t(row_g[lo:hi]), _t(ref_all), 100, 3, True, q=q[lo:hi], km=km[lo:hi], v=v[lo:hi], code=code[lo:hi])
    assert np.array_equal(acc.cpu().numpy(), ref)
    _check_sites((q, km, v, code), c[6:])


@pytest.mark.parametrize("layout", ["i32", "u24"])
def test_extras_and_an_rd_plane_do_not_matter(ctx, layout):
    P, n, E = 130, 7, 9
    recs = records(P, n, 77, extras=E)
    rng = np.random.default_rng(4)
    dup_off = np.concatenate([[0], np.cumsum(np.isin(np.arange(P), rng.choice(P, E, replace=False)))]).astype(np.uint32)
    ext_pos = np.repeat(np.arange(P), np.diff(dup_off.astype(np.int64))).astype(np.uint32)
    rd = np.where(rng.random((n, P + E)) < 0.3, 12345, ABSENT).astype(np.int32)
    full = ctx.records(_pack(ctx, recs, layout), layout, n, E=E, dup_off=_t(dup_off), ext_pos=_t(ext_pos), rd=_t(rd[:, :P]), rd_ext=_t(rd[:, P:]))
    bits = classify(recs[:, :P])
    pl, row_g = _dev(pack_planes(bits, P)), _t(np.arange(n, dtype=np.int32))
    ref = am.reference(recs, bits, P, 100)
    assert ref[0].sum() > 20
    got = ctx.hetsite_reference(full, P, pl, 100)
    assert np.array_equal(got.cpu().numpy(), ref)
    _check_sites(ctx.allelic_sites(full, P, pl, row_g, got, 100, 1, True), am.sites(recs, P, bits, np.arange(n), ref, 100, 1, True))


def test_malformed_planes_are_not_het_sites(ctx):
    """every one of the 64 bit patterns as a plane row: only V + H + exactly two bases is a het site, on the device too"""
    P, n = 256, 4
    recs = ac.small(P, n, 5, layout_max=65534, absent=0.0)
    bits = (np.arange(n * P, dtype=np.int64).reshape(n, P) % 64).astype(np.uint8)
    bits = np.where(np.random.default_rng(6).random((n, P)) < 0.5, bits, classify(recs)).astype(np.uint8)
    pl = pack_planes(bits, P)
    rec = ctx.records(_pack(ctx, recs, "i32"), "i32", n)
    ref = am.reference(recs, bits, P, 100)
    got = ctx.hetsite_reference(rec, P, _dev(pl), 100)
    assert np.array_equal(got.cpu().numpy(), ref) and ref[0].sum() > 50
    exp = am.sites(recs, P, bits, np.arange(n), ref, 100, 1, True)
    assert ((exp[3] >> 3) == am.NOT_HET).sum() > 400
    _check_sites(ctx.allelic_sites(rec, P, _dev(pl), _t(np.arange(n, dtype=np.int32)), got, 100, 1, True), exp)


def test_germline_rows_outside_the_planes_are_none(ctx):
    P, n = 130, 7
    recs, bits, pl, ref, ref_all = _case(P, n)[:5]
    row_g = np.array([-1, n, np.iinfo(np.int32).max, np.iinfo(np.int32).min, 3, 0, 6], np.int32)
    exp = am.sites(recs, P, bits, row_g, ref_all, 100, 3, True)
    assert ((exp[3][:4] >> 3) == am.NOT_HET).all() and (exp[3][:4] & 7 == 7).all() and ((exp[3][4:] >> 3) >= am.TESTED_REF).any()
    # exactly n plane rows: an index of n or beyond would read past the allocation
    _check_sites(ctx.allelic_sites(ctx.records(_pack(ctx, recs, "i32"), "i32", n), P, _dev(pl), _t(row_g), _t(ref_all), 100, 3, True), exp)


@pytest.mark.parametrize("half", [True, False])
def test_reference_gates(ctx, half):
    """CNT at min_normals - 1 and at equality, LO = 0, HI = 0, with and without the fallback"""
    P, n = 130, 7
    recs, bits, pl = _case(P, n)[:3]
    ref = np.zeros((3, 6, P), np.int64)
    k = np.arange(P)
    ref[0] = np.array([4, 5, 6, 5, 5, 0])[k % 6]
    ref[1] = np.array([480, 480, 480, 0, 7, 480])[k % 6]
    ref[2] = np.array([520, 520, 520, 9, 0, 520])[k % 6]
    exp = am.sites(recs, P, bits, np.arange(n), ref, 100, 5, half)
    st = exp[3] >> 3
    assert (st == am.TESTED_REF).any() and (st == (am.TESTED_HALF if half else am.NO_REFERENCE)).any()
    assert not (st == (am.NO_REFERENCE if half else am.TESTED_HALF)).any()
    _check_sites(ctx.allelic_sites(ctx.records(_pack(ctx, recs, "i32"), "i32", n), P, _dev(pl), _t(np.arange(n, dtype=np.int32)), _t(ref), 100, 5, half), exp)


def test_int32_depths(ctx):
    """depths beyond 2^22 and 2^30 and the DEEP status; the reference takes the deep cells as they are"""
    P, n = 130, 7
    c = _case(P, n, True)
    recs, bits, pl, ref, ref_all, row_g = c[:6]
    km, code = c[7], c[9]
    m = km[..., 1].astype(np.int64)
    assert (m > 1 << 22).any() and (m > 1 << 30).any() and ((code >> 3) == am.DEEP).any() and ref[1].max() > 1 << 31
    rec = ctx.records(_pack(ctx, recs, "i32"), "i32", n)
    assert np.array_equal(ctx.hetsite_reference(rec, P, _dev(pl), 100).cpu().numpy(), ref)
    _check_sites(ctx.allelic_sites(rec, P, _dev(pl), _t(row_g), _t(ref_all), 100, 3, True), c[6:])


# ---- stage G, apart, on the model's site planes ------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _planes_for_regions():
    P, n = 1000, 64
    c = _case(P, n)
    return (P, n) + c[6:10]


def _regions(P, R, seed):
    """R lists: empty ones, overlapping ones, repeats, one of more than 256 entries, entries at and beyond P"""
    rng = np.random.default_rng(seed)
    lists = []
    for r in range(R):
        kind = r % 5
        if kind == 0:
            lists.append(np.zeros(0, np.int64))
        elif kind == 1:
            lists.append(np.arange(P)[rng.integers(0, 40):][: int(rng.integers(257, 700))])
        elif kind == 2:
            a = rng.integers(0, P, int(rng.integers(1, 130)))
            lists.append(np.concatenate([a, a[: len(a) // 2]]))  # repeats count twice
        elif kind == 3:
            lists.append(np.concatenate([rng.integers(0, P, 70), [P, P + 1, 2 ** 32 - 1, 2 ** 31]]))
        else:
            lists.append(np.arange(int(rng.integers(0, P - 64)), P)[:64])
    off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    return off, (np.concatenate(lists) if off[-1] else np.zeros(0, np.int64)).astype(np.int64)


@pytest.mark.parametrize("R", [1, 2, 5, 64, 130])
def test_region_sums_equal_the_model(ctx, R):
    P, n, q, km, v, code = _planes_for_regions()
    off, pos = _regions(P, R, R)
    if R == 1:
        off, pos = np.array([0, P + 3]), np.concatenate([np.arange(P), [P, P, P]])  # the whole panel, more than 256 entries
    exp = am.region_sums(q, km, v, code, off, pos, 20.0)
    if R >= 5:
        assert (exp[:, :, am.SITES] > 0).any() and (exp[:, :, am.SIG] > 0).any() and (exp.sum(-1) == 0).any()
    got = ctx.allelic_regions(_t(q), _t(km), _t(v), _t(code), off, pos, 20.0).cpu().numpy()
    assert got.shape == (n, R, 5) and got.dtype == np.int64 and np.array_equal(got, exp)


def test_region_sums_of_a_few_rows_and_cut_offsets(ctx):
    """fewer rows than a strip; offsets beyond W are cut, a falling offset gives an empty list"""
    P, n, q, km, v, code = _planes_for_regions()
    pos = np.arange(0, 600, dtype=np.int64)
    off = np.array([0, 300, 200, 600, 5000], np.int64)
    for rows in (1, 3, 9):
        exp = am.region_sums(q[:rows], km[:rows], v[:rows], code[:rows], off, pos, 13.0)
        dev_off, dev_pos = _t(off.astype(np.uint32).view(np.int32)), _t(pos.astype(np.uint32).view(np.int32))
        got = ctx.allelic_regions(_t(q[:rows]), _t(km[:rows]), _t(v[:rows]), _t(code[:rows]), dev_off, dev_pos, 13.0).cpu().numpy()
        assert np.array_equal(got, exp) and (exp[:, 1] == 0).all() and (exp[:, 0, am.SITES] > 0).any()


def test_repeats_are_bit_identical(ctx):
    P, n = 1000, 64
    c = _case(P, n)
    recs, bits, pl, ref, ref_all, row_g = c[:6]
    rec = ctx.records(_pack(ctx, recs, "u16"), "u16", n)
    off, pos = _regions(P, 64, 3)
    runs = []
    for _ in range(2):
        r = ctx.hetsite_reference(rec, P, _dev(pl), 100)
        s = ctx.allelic_sites(rec, P, _dev(pl), _t(row_g), _t(ref_all), 100, 3, True)
        g = ctx.allelic_regions(*s, off, pos, 20.0)
        runs.append([x.cpu().numpy().tobytes() for x in (r, *s, g)])
    assert runs[0] == runs[1]


def test_planted_cohort_end_to_end(ctx):
    """the encoder, the three stages and the host's verdict on the planted cohort: the model's verdicts, the planted gene found"""
    import ctypes as C

    from amplisolve_amd import host_lib

    co = ac.planted()
    exp = ac.run_model(co)
    P = ac.P
    nrec = ctx.records(_pack(ctx, co["normals"], "u16"), "u16", ac.N_NORMALS)
    trec = ctx.records(_pack(ctx, co["tumours"], "u16"), "u16", ac.N_TUMOURS)
    ref = ctx.hetsite_reference(nrec, P, ctx.genotype_planes(nrec, P), 100)
    assert np.array_equal(ref.cpu().numpy(), exp["ref"])
    s = ctx.allelic_sites(trec, P, ctx.genotype_planes(trec, P), _t(np.arange(ac.N_TUMOURS, dtype=np.int32)), ref, 100, 5, True)
    e = exp["tumours"]
    _check_sites(s, (e["q"], e["km"], e["v"], e["code"], e["q64"]))
    sums = ctx.allelic_regions(*s, co["reg_off"], co["reg_pos"], 20.0).cpu().numpy()
    Q, imb = C.c_double(), C.c_double()
    got = [[host_lib().ampli_host_allelic_region_verdict(np.ascontiguousarray(sums[t, r]).ctypes.data_as(C.c_void_p), 3, 20.0, 0.02, C.byref(Q), C.byref(imb))
            for r in range(sums.shape[1])] for t in range(ac.N_TUMOURS)]
    assert got == [[x[0] for x in row] for row in e["verdicts"]]
    assert got[co["plant"][0]][co["plant"][1]] == am.IMBALANCED
