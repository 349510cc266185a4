"""The row dimension across the grid's y extent: the second launch of every y-split loop, the doubling of genotype_planes' run, and
both sides of every refusal at the grid limit.

Which kernel line produces which shape (tests/scale_shapes.py holds the numbers, tests/test_scale_shapes.py holds them to the sources):
  fdr_adjust       ampli_fdr.hip            `for (int r0 = 0; r0 < rows; r0 += MAX_Y)`: bases d_work + r0 * stride, d_s + r0 * P * 8, d_m + r0,
                                            d_a / d_rank + r0 * P * 4                                    rows = 65535 + 3, P = 5
  dilute           ampli_dilution.hip       `for (int m0 = 0; m0 < n_mix; m0 += MAX_Y)`: mix_base = m0   n_mix = 65535 + 2, P = 17
  pair_score       ampli_paired.hip         `for (long long g0 ...; g0 += MAX_Y)`: pair_base = g0 * 4    n_pairs = 4 * 65535 + 5, P = 1, 65
  nb_score         ampli_overdispersion.hip the same loop: row_base = g0 * 4                             n_t = 4 * 65535 + 5, P = 3
  exceedance       ampli_exceedance.hip     the same loop: row_base = g0 * EX_ROWS                       n_t = 8 * 65535 + 3, P = 3
  genotype_planes  ampli_concordance.hip    `while (... / (GP_WAVES * run) > 65535) run <<= 1;`          n = 65535 * 4 * 16 + 7, P = 1, 65
and the refusals: limit_records / power_records `co.n > 65535`, amplicon_depth_records `strips > 65535`, concordance_pairs `ta > 65535`,
contamination_records `tb > 65535`, poisson_call `(T + PC_SAMPLES - 1) / PC_SAMPLES > 65535`, synth_fill `n_samples > 65535`.

Every input is a base set of a few rows (the features' own cohort builders, bad pairs and bad mixtures kept) repeated along the row
dimension on the device.  These entry points promise that a row's bytes do not depend on its batch, so the expected output is the
base set's, tiled: the first period is held to the model with the feature's own comparison (exact, or its 1e-5), every other row to
its row of the period byte for byte, on the device -- the rows of the second launch (every row from 65535 groups on, the partial last
group included) asserted on their own, so that a failure names the base offset.  No whole output is downloaded.

The refusals: one past the limit the call returns AMPLI_E_RANGE, the message names the limit and every output buffer -- a real buffer
of the refused size, poisoned and fenced -- is untouched; at the limit the call equals the tiled model."""
import ctypes as C

import numpy as np
import pytest

from tests import scale_shapes as sh
from tests.helpers import fenced
from tests.scale_device import assert_tiled, need, release, tile_rows
from tests.test_gpu_loo import _pack
from tests.test_gpu_parity import _t

pytestmark = pytest.mark.gpu
Y = sh.Y
E_RANGE = -6
ABSENT = np.iinfo(np.int32).min


def _nbytes(*shapes_and_sizes):
    return sum(int(np.prod(s)) * e for s, e in shapes_and_sizes)


# ==== A. the second launch ==============================================================================================================

@pytest.mark.parametrize("two_sided", [False, True])
def test_fdr_adjust_second_launch(ctx, two_sided):
    from tests import fdr_model as fm
    from tests import fdr_planes as fp

    rows, (P,) = sh.SPLITS["fdr_adjust"]["rows"], sh.SPLITS["fdr_adjust"]["P"]
    s, A, m, R = fp.case(P, two_sided)  # one row per kind of plane
    b = s.shape[0]
    need(ctx, _nbytes(((rows, P, 8), 4), ((rows, P, 4), 8), ((rows,), 4)) + ctx.fdr_workspace_bytes(rows, P))
    d_s = tile_rows(_t(s.copy()), rows)
    a, mm, rk = ctx.fdr_adjust(d_s, two_sided, rank=True)
    ctx.sync()
    fm.compare(a[:b].cpu().numpy(), mm[:b].cpu().numpy(), rk[:b].cpu().numpy(), A, m, R)
    for name, t in (("a", a), ("m", mm), ("rank", rk)):
        assert_tiled(t, t[:b].clone(), Y, f"fdr_adjust {name}")
    assert_tiled(d_s, _t(s.copy()), None, "fdr_adjust: the plane is never written")
    del d_s, a, mm, rk
    release()


def test_dilute_second_launch(ctx):
    from tests.dilution_cohorts import ROWS_A, ROWS_B, case
    from tests.dilution_model import BAD_MIXTURE, KEEP_ALL, dilute_model, keep_of
    from tests.test_gpu_dilution import _records

    n_mix, (P,) = sh.SPLITS["dilute"]["rows"], sh.SPLITS["dilute"]["P"]
    A, B, mix, _, _ = case(P, 9, "different")
    key = 0xD11A7E0000000001
    mix = list(mix) + [(ROWS_A, 0, keep_of(0.5), keep_of(0.5), key), (0, ROWS_B, keep_of(0.5), keep_of(0.5), key), (0, -2, 5, 5, key),
                       (1, -1, KEEP_ALL + 1, 0, key)]  # the bad mixtures stay in the base set
    want, want_flags = dilute_model(A[0], B[0], P, mix)
    b = len(mix)
    assert b == 13 and (want_flags[9:] == BAD_MIXTURE).all() and not want_flags[:9].any() and (want[:9, :, 0] != ABSENT).any()
    need(ctx, _nbytes(((n_mix, P, 8), 4), ((n_mix, 4), 8), ((n_mix,), 4)) * 2)
    words = np.array([[(ra & 0xFFFFFFFF) | (rb & 0xFFFFFFFF) << 32, ka, kb, k & 0xFFFFFFFFFFFFFFFF] for ra, rb, ka, kb, k in mix], dtype=np.uint64)
    d_mix = tile_rows(_t(words.view(np.int64)), n_mix)
    out, flags = ctx.dilute(_records(ctx, A, P, "u16", pad=3), _records(ctx, B, P, "u24"), P, d_mix)
    ctx.sync()
    assert_tiled(out, _t(np.array(want, np.int32)), Y, "dilute out")
    assert_tiled(flags, _t(np.array(want_flags, np.int32)), Y, "dilute flags")
    del d_mix, out, flags
    release()


@pytest.mark.parametrize("P", sh.SPLITS["pair_score"]["P"])
def test_pair_score_second_launch(ctx, P):
    from tests.dispersion_cohorts import cohort
    from tests.paired_model import NA, score_model
    from tests.test_gpu_paired import CUTOFF, ROWS_A, ROWS_B, _pairs, _records, _same

    n_pairs = sh.SPLITS["pair_score"]["rows"]
    rng = np.random.default_rng(31 * P)
    A = cohort(P, ROWS_A, 3 * P + 77, extras=True, own_rd=True, u16=True)
    B = cohort(P, ROWS_B, 5 * P + 78, extras=True, own_rd=True, u16=True)
    ref = rng.integers(0, 4, P).astype(np.uint8)
    if P > 8:
        ref[rng.random(P) < 0.08] = 255
    pairs = _pairs("different", 9, rng) + [(ROWS_A, 0), (1, -1)]  # the bad pairs stay in the base set
    b = len(pairs)
    assert b == 11 and n_pairs % b != 0  # 11 and 4 are coprime: every pair of the base set meets every wave of a workgroup
    want, want64 = score_model(A[0], B[0], P, pairs, ref, CUTOFF)
    assert (want[9:] == NA).all() and (P == 1 or (want[:9] != NA).any())
    need(ctx, _nbytes(((n_pairs, P, 8), 4)) * 2)
    d_pairs = tile_rows(_t(np.array(pairs, np.int32)), n_pairs)
    s = ctx.pair_score(_records(ctx, A, P, "u16", pad=3), _records(ctx, B, P, "u16"), P, d_pairs, _t(ref), CUTOFF)
    ctx.sync()
    _same(s[:b].cpu().numpy(), want, want64)
    assert_tiled(s, s[:b].clone(), 4 * Y, f"pair_score s, P = {P}")
    del d_pairs, s
    release()


@pytest.mark.parametrize("with_omega", [False, True])
def test_nb_score_second_launch(ctx, with_omega):
    from tests.test_gpu_overdispersion import CUTOFF, NA, Q_TOL, _q_case

    n_t, (P,) = sh.SPLITS["nb_score"]["rows"], sh.SPLITS["nb_score"]["P"]
    b = 7
    recs, ref, thr, omega, q0_m, q_m, _ = _q_case(P, b)
    want = q_m if with_omega else q0_m
    assert n_t % b != 0 and (want != NA).any() and (want == NA).any()
    need(ctx, _nbytes(((n_t, P, 8), 4), ((n_t, P, 8), 2)) * 2)
    d_recs = tile_rows(_pack(ctx, recs, "u16"), n_t)
    q = ctx.nb_score(ctx.records(d_recs, "u16", n_t), P, _t(thr), _t(ref), _t(omega) if with_omega else None, CUTOFF)
    ctx.sync()
    got = q[:b].cpu().numpy()
    exact = (want == NA) | (want == np.float32(-888)) | (want == 0)
    assert np.array_equal(got[exact], want[exact]) and np.array_equal(got == NA, want == NA)
    assert (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= Q_TOL).all()
    assert_tiled(q, q[:b].clone(), 4 * Y, "nb_score q")
    del d_recs, q
    release()


@pytest.mark.parametrize("accumulate", [0, 1])
def test_exceedance_second_launch(ctx, accumulate):
    from tests.exceedance_model import NA
    from tests.test_gpu_exceedance import _case

    n_t, (P,) = sh.SPLITS["exceedance"]["rows"], sh.SPLITS["exceedance"]["P"]
    b, n_n = 7, sh.EXCEEDANCE_NORMALS
    t, n, ref, e, g = _case(P, b, n_n)
    assert n_t % b != 0 and (g != NA).any() and (g == NA).any() and (e > 0).any()
    need(ctx, _nbytes(((n_t, P, 9), 2), ((n_t, P, 8), 2)) * 2)
    rt = ctx.records(tile_rows(_pack(ctx, t, "u16"), n_t), "u16", n_t)
    rn = ctx.records(_pack(ctx, n, "u24"), "u24", n_n)
    d_e, d_g = _t(np.array(e.view(np.int16))), _t(np.array(g.view(np.int16)))  # copies: the shared case is read-only
    if accumulate:  # onto the tiled counts of an earlier chunk of the same normals: every count doubles, NA stays NA
        elig, ge = ctx.exceedance(rt, rn, P, _t(ref), accumulate=True, elig=tile_rows(d_e, n_t), ge=tile_rows(d_g, n_t))
        d_e, d_g = _t((2 * e).view(np.int16)), _t(np.where(g == NA, NA, 2 * g).astype(np.uint16).view(np.int16))
    else:
        elig, ge = ctx.exceedance(rt, rn, P, _t(ref))
    ctx.sync()
    assert_tiled(elig, d_e, 8 * Y, f"exceedance elig, accumulate = {accumulate}")
    assert_tiled(ge, d_g, 8 * Y, f"exceedance ge, accumulate = {accumulate}")
    del rt, elig, ge
    release()


@pytest.mark.parametrize("P", sh.GENOTYPE["P"])
def test_genotype_planes_doubled_run(ctx, P):
    from tests.concordance_cohorts import records
    from tests.concordance_model import planes, words

    n, b = sh.GENOTYPE["rows"], 7
    recs = records(P, b, 900 + P)
    exp = planes(recs, P)
    assert n % b != 0 and exp.any()
    need(ctx, _nbytes(((n, P, 8), 2), ((n, 6, words(P)), 8)) + (256 << 20))
    d_recs = tile_rows(_pack(ctx, recs, "u16"), n)
    out = ctx.genotype_planes(ctx.records(d_recs, "u16", n), P)
    ctx.sync()
    # the rows from 65535 groups of the initial run on: the ones a launch that did not double the run would leave unwritten
    assert_tiled(out, _t(np.array(exp.view(np.int64))), Y * 4 * 16, f"genotype_planes, P = {P}", second="the grid's last y step at the doubled run")
    del d_recs, out
    release()


# ==== B. the refusals at the grid limit, both sides ====================================================================================

def _refused(ctx, rc, limit, *checks):
    """rc is AMPLI_E_RANGE, the message names the limit, and every byte of every fenced output still holds its poison"""
    import torch

    msg = ctx.lib.ampli_last_error(ctx.h).decode()
    assert rc == E_RANGE, (rc, msg)
    assert str(limit) in msg, msg
    torch.cuda.synchronize()
    for check in checks:
        assert bool((check.raw == 0xFF).all()), "a refused call wrote to an output"
    assert ctx.flags() == 0


def _raises_range(ctx, limit, call, *checks):
    """the same through a wrapper of Context that raises"""
    from amplisolve_amd import AmpliError

    with pytest.raises(AmpliError) as e:
        call()
    assert f"({E_RANGE})" in str(e.value), str(e.value)
    _refused(ctx, E_RANGE, limit, *checks)


LIMIT_P = 1
LIMIT_RECS = np.array([[[1990, 10, 0, 0, 1985, 15, 0, 0]], [[ABSENT, 0, 0, 0, 0, 0, 0, 0]], [[50, 0, 0, 0, 60, 0, 0, 0]], [[5000, 0, 3, 100, 5000, 1, 0, 90]],
                       [[300, 5, 5, 5, 280, 6, 7, 8]], [[65534, 0, 0, 0, 65534, 0, 0, 0]], [[101, 0, 0, 0, 99, 0, 0, 0]]], np.int32)
LIMIT_THR = np.array([0.002, 0.002, -1.0, 1.5, 0.002, 0.01, 0.002, 0.002], np.float32).reshape(2, 4, 1)
LIMIT_REF = np.zeros(1, np.uint8)
LEVELS = (0.01, 0.05)


def _limit_base():
    from tests import limit_model as lm

    exp = lm.limit_model(LIMIT_RECS, LIMIT_P, LIMIT_THR, LIMIT_REF, 100, levels=LEVELS, from_one=False)
    assert {lm.OK, lm.REF, lm.LOWDEPTH, lm.NOESTIMATE, lm.UNREACHABLE, lm.ABSENT_CODE} <= set(np.unique(exp["status"] & 7).tolist())
    return exp


def test_limit_records_at_the_grid_limit(ctx):
    import torch

    from tests import limit_model as lm

    n, b = sh.LIMITS["limit_records"], len(LIMIT_RECS)
    exp = _limit_base()
    base = _pack(ctx, LIMIT_RECS, "u16")
    d_thr, d_ref = _t(LIMIT_THR), _t(LIMIT_REF)
    res = ctx.detection_limits(ctx.records(tile_rows(base, n), "u16", n), LIMIT_P, d_thr, d_ref, 100, LEVELS)
    ctx.sync()
    got = {k: res[k][:b].cpu().numpy() for k in ("min_reads", "status", "counts")}
    lm.settle(got, LIMIT_RECS, LIMIT_P, LIMIT_THR, LIMIT_REF, 100, levels=LEVELS)
    for k in got:
        assert np.array_equal(got[k], exp[k]), k
        assert_tiled(res[k], res[k][:b].clone(), None, f"limit_records {k}")
    # one past the limit
    n += 1
    lv = torch.tensor(LEVELS, dtype=torch.float32, device="cuda")
    (mr, c0), (st, c1), (cn, c2) = fenced((n, 1, 4, 2), torch.int32), fenced((n, 1, 4), torch.uint8), fenced((n, 6 + len(LEVELS)), torch.int64)
    rec = ctx.records(tile_rows(base, n), "u16", n)
    rc = ctx.lib.ampli_limit_records(ctx.h, C.byref(rec), LIMIT_P, C.c_void_p(d_thr.data_ptr()), C.c_void_p(d_ref.data_ptr()), 100, C.c_void_p(lv.data_ptr()),
                                     len(LEVELS), C.c_void_p(mr.data_ptr()), C.c_void_p(st.data_ptr()), C.c_void_p(cn.data_ptr()))
    _refused(ctx, rc, sh.LIMITS["limit_records"], c0, c1, c2)


def test_power_records_at_the_grid_limit(ctx):
    import torch

    from tests import limit_model as lm
    from tests import power_model as pm
    from tests.test_gpu_power import LOD_TOL, TAIL_TOL, _host

    n, b = sh.LIMITS["power_records"], len(LIMIT_RECS)
    exp = _limit_base()
    status, min_reads = exp["status"], exp["min_reads"]
    FW, BW = LIMIT_RECS[:, :, :4].astype(np.int64).sum(-1), LIMIT_RECS[:, :, 4:].astype(np.int64).sum(-1)
    ok = pm.is_ok(status, min_reads, FW, BW)
    assert ok.sum() >= 4 and (~ok).sum() >= 8
    base = _pack(ctx, LIMIT_RECS, "u16")
    d_mr, d_st = tile_rows(_t(min_reads), n + 1), tile_rows(_t(status), n + 1)
    res = ctx.detection_power(ctx.records(tile_rows(base, n), "u16", n), LIMIT_P, d_mr[:n], d_st[:n], LEVELS, 0.95)
    ctx.sync()
    power, lod = res["power"][:b].cpu().numpy(), res["lod"][:b].cpu().numpy()
    assert (power[~ok] == 0).all() and (lod[~ok] == 0).all()
    for cell in (tuple(x) for x in np.argwhere(ok)):
        pw, ld = _host(int(FW[cell[:2]]), int(min_reads[cell][0]), int(BW[cell[:2]]), int(min_reads[cell][1]), LEVELS, 0.95)
        assert np.abs(power[cell] - np.array(pw)).max() <= TAIL_TOL and abs(float(lod[cell]) / ld - 1) <= LOD_TOL
    for k in ("power", "lod", "counts"):
        assert_tiled(res[k], res[k][:b].clone(), None, f"power_records {k}")
    assert int(res["counts"][:b, 0].sum()) == int(ok.sum())
    n += 1
    lv = torch.tensor(LEVELS, dtype=torch.float32, device="cuda")
    (pw_, c0), (ld_, c1), (cn, c2) = fenced((n, 1, 4, len(LEVELS)), torch.float32), fenced((n, 1, 4), torch.float32), fenced((n, 1 + len(LEVELS)), torch.int64)
    rec = ctx.records(tile_rows(base, n), "u16", n)
    rc = ctx.lib.ampli_power_records(ctx.h, C.byref(rec), LIMIT_P, C.c_void_p(d_mr.data_ptr()), C.c_void_p(d_st.data_ptr()), C.c_void_p(lv.data_ptr()),
                                     len(LEVELS), 0.95, C.c_void_p(pw_.data_ptr()), C.c_void_p(ld_.data_ptr()), C.c_void_p(cn.data_ptr()))
    _refused(ctx, rc, sh.LIMITS["power_records"], c0, c1, c2)


def test_amplicon_depth_records_at_the_grid_limit(ctx):
    import torch

    from tests.amplicon_model import depth_sums

    n, P = sh.LIMITS["amplicon_depth_records"], 3
    recs = np.concatenate([LIMIT_RECS, LIMIT_RECS[::-1], np.roll(LIMIT_RECS, 3, axis=0)], axis=1)  # [7, 3, 8]
    amp_off, amp_pos = np.array([0, 2, 2, 4]), np.array([0, 2, 1, 1])  # an empty list; a position listed twice
    want = depth_sums(recs, amp_off, amp_pos, 100)
    assert want[:, 0].any() and not want[:, 1].any()
    base = _pack(ctx, recs, "u16")
    out = ctx.amplicon_depth(ctx.records(tile_rows(base, n), "u16", n), P, amp_off, amp_pos, 100)
    ctx.sync()
    assert_tiled(out, _t(want), None, "amplicon_depth_records")
    del out
    n += 1
    sums, check = fenced((n, 3, 4), torch.int64)
    _raises_range(ctx, sh.LIMITS["amplicon_depth_records"], lambda: ctx.amplicon_depth(ctx.records(tile_rows(base, n), "u16", n), P, amp_off, amp_pos, 100, out=sums), check)
    del sums, check
    release()


def test_concordance_pairs_at_the_grid_limit(ctx):
    import torch

    from tests.concordance_cohorts import records
    from tests.concordance_model import classify, pack_planes, pair_counts

    n_a, n_b, P, b = sh.LIMITS["concordance_pairs"], 3, 65, 7
    bits = classify(records(P, b + n_b, 4242))
    pl = pack_planes(bits, P)
    want = pair_counts(bits[:b], bits[b:])
    assert want[:, :, 0].any()
    need(ctx, _nbytes(((n_a + 1, 6, 2), 8), ((n_a + 1, n_b, 5), 4)) * 2)
    d_b = _t(pl[b:].view(np.int64))
    d_a = tile_rows(_t(pl[:b].view(np.int64)), n_a + 1)
    out = ctx.concordance(d_a[:n_a], d_b, P)
    ctx.sync()
    assert_tiled(out, _t(want.astype(np.int32)), None, "concordance_pairs")
    del out
    counts, check = fenced((n_a + 1, n_b, 5), torch.int32)
    rc = ctx.lib.ampli_concordance_pairs(ctx.h, P, C.c_void_p(d_a.data_ptr()), n_a + 1, C.c_void_p(d_b.data_ptr()), n_b, C.c_void_p(counts.data_ptr()))
    _refused(ctx, rc, sh.LIMITS["concordance_pairs"], check)
    del counts, check, d_a
    release()


def test_contamination_records_at_the_grid_limit(ctx):
    import torch

    from tests import contamination_model as cm
    from tests.concordance_cohorts import records
    from tests.concordance_model import classify, pack_planes

    n_b, P, b = sh.LIMITS["contamination_records"], 65, 7
    recs = records(P, 1 + b, 5151)
    bits = classify(recs)
    pl = pack_planes(bits, P)
    want = cm.sums(recs[:1], bits[:1], bits[1:])  # one recipient, seven sources
    assert want.any()
    need(ctx, _nbytes(((n_b + 1, 6, 2), 8), ((n_b + 1, 9), 8)) * 2)
    rec = ctx.records(_pack(ctx, recs[:1], "u16"), "u16", 1)
    d_a = _t(pl[:1].view(np.int64))
    d_b = tile_rows(_t(pl[1:].view(np.int64)), n_b + 1)
    out = ctx.contamination(rec, P, d_a, d_b[:n_b])
    ctx.sync()
    assert_tiled(out[0], _t(want[0]), None, "contamination_records")
    del out
    release()
    sums, check = fenced((1, n_b + 1, 9), torch.int64)
    _raises_range(ctx, sh.LIMITS["contamination_records"], lambda: ctx.contamination(rec, P, d_a, d_b, out=sums), check)
    del sums, check, d_b
    release()


def test_poisson_call_at_the_grid_limit(ctx):
    import torch

    from amplisolve_amd.api import POISSON_FULL, POISSON_PREFILTER
    from oracle import pyoracle as orc

    T, P, b = sh.LIMITS["poisson_call"], 3, 7
    trecs = np.concatenate([LIMIT_RECS, LIMIT_RECS[::-1], np.roll(LIMIT_RECS, 3, axis=0)], axis=1)
    thr = np.array([float(f"{x:f}") for x in np.random.default_rng(3).uniform(2e-4, 0.01, 8 * P)], np.float32).reshape(2, 4, P)
    ref = np.array([0, 1, 0], np.uint8)
    exp = orc.poisson_call(trecs, P, thr, ref, 100)
    assert exp["call_mask"].any() and not exp["call_mask"].all()
    d_thr, d_ref = _t(thr), _t(ref)
    d_recs = tile_rows(_t(trecs), T + 1)
    d_mask, d_q = _t(exp["call_mask"]), None
    # the base set queues far more of its records than a cohort does, and a panel of three positions fills one tile in eight: its items meet
    # in four of the 32 shards.  Room for all of them, so that AMPLI_FLAG_QUEUE_OVERFLOW stays down
    ctx.set_queue_items(8 * T * P)
    try:
        for mode in (POISSON_PREFILTER, POISSON_FULL):
            res = ctx.poisson_call(d_recs[:T], P, d_thr, d_ref, 100, mode=mode, dense_q=mode == POISSON_FULL)
            ctx.sync()
            assert ctx.flags() == 0
            assert_tiled(res["call_mask"], d_mask, None, f"poisson_call mask, mode {mode}")
            if mode == POISSON_FULL:
                q = res["q"][:b].cpu().numpy()
                assert np.array_equal(q == -1, exp["q"] == -1) and np.max(np.abs(q - exp["q"])) <= 1e-5
                assert_tiled(res["q"], res["q"][:b].clone(), None, "poisson_call q")
            del res
    finally:
        ctx.set_queue_items(0)
    T += 1
    raw_mask, c0 = fenced(((T * P + 3) // 4 * 4,), torch.uint8)
    q, c1 = fenced((T, P, 4, 2), torch.float64)
    for mode in (POISSON_PREFILTER, POISSON_FULL):
        _raises_range(ctx, sh.LIMITS["poisson_call"],
                      lambda: ctx.poisson_call(d_recs, P, d_thr, d_ref, 100, mode=mode, call_mask=raw_mask[:T * P].view(T, P), q=q if mode == POISSON_FULL else None), c0, c1)
    del d_recs, q, raw_mask
    release()


def test_synth_fill_at_the_grid_limit(ctx):
    import torch

    from tests.helpers import synth_recs

    n, P = sh.LIMITS["synth_fill"], 3
    got = ctx.synth_fill(P, n, first_sample=5, depth=2000, tumour=True)
    ctx.sync()
    assert torch.equal(got, _t(synth_recs(P, n, first=5, depth=2000, tumour=True)))
    out, check = fenced((n + 1, P, 8), torch.int32)
    _raises_range(ctx, sh.LIMITS["synth_fill"], lambda: ctx.synth_fill(P, n + 1, out=out), check)
