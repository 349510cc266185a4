"""Context.panel_dispersion (dispersion_stream_kernel, dispersion_sample_reduce_kernel, dispersion_finalize_kernel) against the exact
definition (tests/dispersion_model.py): every record layout, chunked cohorts, extra occurrences, lines with their own RD column, S from
1 to 64, P not a multiple of 64; counts at the 16-bit layout's maximum; bit-identical repeats; a planted contaminated normal.
The tolerances are DESIGN 13's: a forward bound of the fp64 arithmetic, not what the kernel happens to give."""
import numpy as np
import pytest

from tests.dispersion_cohorts import cohort_and_model, planted
from tests.dispersion_model import FEW, HIGH, dispersion_model
from tests.test_gpu_loo import _pack
from tests.test_gpu_parity import _t

pytestmark = pytest.mark.gpu
ABSENT = np.iinfo(np.int32).min
Z_CUTOFF = 4.0


def _gpu(ctx, recs, P, E, dup_off, ext_pos, rd, layout, cuts, cov, z_cutoff=Z_CUTOFF, samples=True):
    """pass 1: the whole cohort's C = 0 table, chunk by chunk; pass 2: panel_dispersion over the resident chunks"""
    acc0 = ctx.new_acc(P)
    chunks = []
    for ci in range(len(cuts) - 1):
        lo, hi = cuts[ci], cuts[ci + 1]
        kw = {}
        if E:
            kw.update(dup_off=_t(dup_off), ext_pos=_t(ext_pos))
        if rd is not None:
            kw.update(rd=_t(rd[lo:hi, :P]), rd_ext=_t(rd[lo:hi, P:]) if E else None)
        rec = ctx.records(_pack(ctx, recs[lo:hi], layout), layout, hi - lo, E=E, **kw)
        ctx.error_reduce_records(rec, P, acc0, 0.0, cov, first_sample=lo, accumulate=ci > 0, summary=True)
        chunks.append(rec)
    res = ctx.panel_dispersion(chunks, P, acc0, cov, z_cutoff, samples=samples)
    out = {k: (v.cpu().numpy() if v is not None else None) for k, v in res.items()}
    out["K"] = acc0.snt.cpu().numpy()
    out["D"] = acc0.srd.cpu().numpy()
    out["n"] = acc0.cnt.cpu().numpy()
    return out


def _check(got, exp, z_cutoff=Z_CUTOFF, samples=True):
    assert np.array_equal(got["K"], exp["K"].astype(np.float64)) and np.array_equal(got["D"], exp["D"]) and np.array_equal(got["n"], exp["n"])
    K = exp["K"].astype(np.float64)
    few = exp["status"] == FEW
    assert np.array_equal(got["status"] & 7, exp["status"] & 7)
    for k in ("x2", "rinv", "z", "phi"):
        assert (got[k][few] == 0).all(), k
    dx, dz = np.abs(got["x2"] - exp["x2"]), np.abs(got["z"] - exp["z"])
    dr = np.abs(got["rinv"] - exp["rinv"])
    dp = np.abs(got["phi"].astype(np.float64) - exp["phi"].astype(np.float64))
    print(f"X2 {np.max(dx / (1 + K + exp['x2'])):.3g} of (1 + K + X2), z {np.max(dz / (1 + K + np.abs(exp['z']))):.3g} of (1 + K + |z|), "
          f"sum 1/d {np.max(dr[~few] / exp['rinv'][~few], initial=0):.3g} relative, phi {np.max(dp[~few] / np.maximum(np.abs(exp['phi'][~few]), 1e-30), initial=0):.3g} relative")
    assert (dx <= 1e-12 * (1 + K + exp["x2"])).all()
    assert (dz <= 1e-12 * (1 + K + np.abs(exp["z"]))).all()
    assert (dr <= 1e-12 * exp["rinv"]).all()
    assert (dp <= 2e-7 * np.abs(exp["phi"].astype(np.float64))).all()
    band = ~few & (np.abs(exp["z"] - z_cutoff) <= 1e-9 * (1 + np.abs(exp["z"])))
    assert band.sum() < 0.01 * max(1, (~few).sum())
    assert np.array_equal((got["status"] & HIGH)[~band], (exp["status"] & HIGH)[~band])
    assert ((got["status"] & ~np.uint8(HIGH | 7)) == 0).all()
    high = np.where(band, got["status"], exp["status"]) & HIGH != 0  # the model's flags, the device's own inside the band
    assert got["counts"].tolist() == [int((~few).sum()), int(few.sum()), int(high.sum()), int(high.any(axis=(0, 1)).sum())]
    if samples:
        assert np.array_equal(got["sample_terms"], exp["sample_terms"])
        sx = np.abs(got["sample_x2"] - exp["sample_x2"])
        se = np.abs(got["sample_expect"] - exp["sample_expect"])
        print(f"sample_x2 {np.max(sx / (1 + exp['sample_x2'] + exp['sample_scale'])):.3g} of its scale, sample_expect {np.max(se / (1 + exp['sample_terms'])):.3g} of (1 + terms)")
        assert (sx <= 1e-10 * (1 + exp["sample_x2"] + exp["sample_scale"])).all()
        assert (se <= 1e-10 * (1 + exp["sample_terms"])).all()


# test_gpu_loo.py's shapes: (P, S, chunk cuts, extras, own RD column, coverage_cutoff); an RD plane goes with the 32- and 24-bit layouts only
SHAPES = [(300, 7, (0, 7), False, False, 100), (300, 7, (0, 3, 7), True, False, 30), (1000, 64, (0, 20, 41, 64), True, True, 100),
          (130, 2, (0, 1, 2), True, False, 1), (77, 1, (0, 1), False, False, 100)]
CASES = [(lay,) + sh for lay in ("i32", "u24", "u16") for sh in SHAPES if not (lay == "u16" and sh[4])]


@pytest.mark.parametrize("layout,P,S,cuts,extras,own_rd,cov", CASES)
def test_dispersion_equals_the_model(ctx, layout, P, S, cuts, extras, own_rd, cov):
    (recs, E, dup_off, ext_pos, rd), exp = cohort_and_model(P, S, P + S, extras, own_rd, True, cov)  # counts <= 65534: one cohort for every layout
    n_ok = int((exp["status"] != FEW).sum())
    if S >= 7:
        assert n_ok >= 0.1 * 6 * P  # the model has OK cells at all: a tenth of the non-reference cells
    if S == 1:
        assert n_ok == 0
    got = _gpu(ctx, recs, P, E, dup_off, ext_pos, rd, layout, cuts, cov)
    _check(got, exp)
    if S == 1:  # every cell FEW: every output is 0
        for k in ("x2", "rinv", "z", "phi", "sample_x2", "sample_expect", "sample_terms"):
            assert (got[k] == 0).all(), k
        assert got["counts"].tolist() == [0, 8 * P, 0, 0]


def test_u16_counts_at_the_layouts_maximum(ctx):
    """records whose major count is 65 534, the largest the 16-bit layout holds (65 535 in field 0 is its absent mark)"""
    P, S = 200, 9
    (recs, E, dup_off, ext_pos, rd), _ = cohort_and_model(P, S, 11, True, False, True, 100)
    recs = recs.copy()
    rng = np.random.default_rng(8)
    for s, r in zip(rng.integers(0, S, 400), rng.integers(0, P + E, 400)):
        if recs[s, r, 0] == ABSENT:
            continue
        for st in range(2):
            recs[s, r, st * 4 + int(np.argmax(recs[s, r, st * 4:st * 4 + 4]))] = 65534
    recs[0, 0] = [65534, 3000, 1, 0, 65534, 2900, 0, 2]  # field 0 at the maximum, a second base just under 5 %
    exp = dispersion_model(recs, P, 100, E=E, ext_pos=ext_pos, z_cutoff=Z_CUTOFF)
    assert (exp["D"] > 65534).any() and (exp["status"] != FEW).sum() >= 0.1 * 6 * P
    _check(_gpu(ctx, recs, P, E, dup_off, ext_pos, rd, "u16", (0, 4, 9), 100), exp)


def test_repeats_are_bit_identical_and_chunkings_agree(ctx):
    P, S = 1000, 64
    (recs, E, dup_off, ext_pos, rd), exp = cohort_and_model(P, S, P + S, True, True, True, 100)
    a = _gpu(ctx, recs, P, E, dup_off, ext_pos, rd, "u24", (0, 20, 41, 64), 100)
    b = _gpu(ctx, recs, P, E, dup_off, ext_pos, rd, "u24", (0, 20, 41, 64), 100)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    c = _gpu(ctx, recs, P, E, dup_off, ext_pos, rd, "u24", (0, 64), 100)
    _check(c, exp)
    assert np.array_equal(a["status"] & 7, c["status"] & 7) and np.array_equal(a["sample_terms"], c["sample_terms"])


def test_without_sample_arrays(ctx):
    P, S = 300, 7
    (recs, E, dup_off, ext_pos, rd), exp = cohort_and_model(P, S, P + S, True, False, True, 30)
    got = _gpu(ctx, recs, P, E, dup_off, ext_pos, rd, "i32", (0, 3, 7), 30, samples=False)
    assert got["sample_x2"] is None
    _check(got, exp, samples=False)


def test_planted_normal_is_found_on_the_device(ctx):
    recs, spots = planted()
    S, P = recs.shape[0], recs.shape[1]
    got = _gpu(ctx, recs, P, 0, None, None, None, "u16", (0, 6, 11), 100)
    _check(got, dispersion_model(recs, P, 100, z_cutoff=Z_CUTOFF))
    for p, nt in spots:
        assert got["status"][0, nt, p] & HIGH and got["status"][1, nt, p] & HIGH, (p, nt)
    ratio = got["sample_x2"] / got["sample_expect"]
    assert int(np.argmax(ratio)) == 4 and np.delete(ratio, 4).max() <= 0.5 * ratio[4]
