"""Context.overdispersion_sums, overdispersion_fit and nb_score (overdispersion_stream_kernel, overdispersion_finalize_kernel,
nb_score_kernel) against the definition (tests/overdispersion_model.py).  S2 is exact for uint16 cohorts (integers below 2^53) and
within 1e-12 where int32 depths carry the sum beyond 64 bits; omega is held to the forward bound of its five roundings; Q to 1e-5
(tests/test_overdispersion_host.py derives it), NA, -888 and 0 exactly."""
import functools
import os

import numpy as np
import pytest

from tests.dispersion_cohorts import cohort
from tests.dispersion_model import HIGH
from tests.helpers import GOLDEN
from tests.overdispersion_cohorts import COV, C_VALUE, Z_CUTOFF, planted_and_fit, tally
from tests.overdispersion_model import decisions, omega_model, s2_model, score_model
from tests.test_gpu_loo import _pack
from tests.test_gpu_parity import _t

pytestmark = pytest.mark.gpu
ABSENT = np.iinfo(np.int32).min
Q_TOL = 1e-5
NA = np.float32(-1)


# ---- S2 ----------------------------------------------------------------------------------------------------------------------------------

def _chunks(ctx, recs, P, E, dup_off, ext_pos, rd, layout, cuts, pad=0):
    out = []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        kw = {}
        if E:
            kw.update(dup_off=_t(dup_off), ext_pos=_t(ext_pos))
        if rd is not None:
            kw.update(rd=_t(rd[lo:hi, :P]), rd_ext=_t(rd[lo:hi, P:]) if E else None)
        part = recs[lo:hi]
        if pad:  # a padded row stride: the rows are pad records longer than P + E
            filler = np.full((hi - lo, pad, 8), 12345, np.int32)
            part = np.concatenate([part, filler], axis=1)
        out.append(ctx.records(_pack(ctx, part, layout), layout, hi - lo, E=E, row_stride=P + E + pad if pad else 0, **kw))
    return out


def _cuts(n, parts):
    return tuple(sorted(set(int(round(i * n / parts)) for i in range(parts + 1))))


@functools.lru_cache(maxsize=None)
def _s2_case(P, n):
    recs, E, dup_off, ext_pos, rd = cohort(P, n, 3 * P + n, extras=True, own_rd=True, u16=True)  # positions listed twice, absent records, an RD plane
    return (recs, E, dup_off, ext_pos, rd), s2_model(recs, P, 30, E=E, ext_pos=ext_pos)


@pytest.mark.parametrize("layout", ["i32", "u24", "u16"])
@pytest.mark.parametrize("P,n", [(1, 1), (63, 2), (64, 3), (65, 5), (130, 9), (1000, 33)])
def test_s2_equals_the_model(ctx, layout, P, n):
    (recs, E, dup_off, ext_pos, rd), exp = _s2_case(P, n)
    if layout == "u16":
        rd = None  # an RD plane goes with the 32- and 24-bit layouts only; it plays no part in the gate of these records
    want = exp.astype(np.float64)
    assert (exp < 2 ** 53).all()
    if n >= 5:
        assert (want > 0).sum() >= 0.5 * 8 * P
    acc0 = ctx.new_acc(P)
    got = {}
    for parts in (1, 2, 5):
        cuts = _cuts(n, min(parts, n))
        ch = _chunks(ctx, recs, P, E, dup_off, ext_pos, rd, layout, cuts, pad=3 if parts == 2 else 0)
        got[parts] = ctx.overdispersion_sums(ch, P, acc0, 30).cpu().numpy()
        assert np.array_equal(got[parts], want), parts
    again = ctx.overdispersion_sums(_chunks(ctx, recs, P, E, dup_off, ext_pos, rd, layout, _cuts(n, min(5, n))), P, acc0, 30).cpu().numpy()
    assert again.tobytes() == got[5].tobytes()


def test_s2_beyond_64_bits(ctx):
    """int32 depths next to 2^30: a square is 2^60, 33 records carry the sum into the second word; one rounding per word and one of their sum"""
    P, n = 65, 33
    rng = np.random.default_rng(5)
    recs = np.zeros((n, P, 8), np.int64)
    d = rng.integers(2 ** 26, 2 ** 30 - 2000, size=(n, P, 2))
    d[:, : P // 2] = 2 ** 30 - 2000 - rng.integers(0, 50, size=(n, P // 2, 2))
    alt = rng.integers(0, 40, size=(n, P, 2, 3))
    for st in range(2):
        recs[:, :, st * 4] = d[:, :, st] - alt[:, :, st].sum(-1)
        recs[:, :, st * 4 + 1:st * 4 + 4] = alt[:, :, st]
    recs = recs.astype(np.int32)
    recs[3, 7, 0] = ABSENT
    exp = s2_model(recs, P, 100)
    assert max(int(v) for v in exp.ravel()) > 2 ** 64 and min(int(v) for v in exp[:, 1].ravel()) > 2 ** 53
    got = ctx.overdispersion_sums(_chunks(ctx, recs, P, 0, None, None, None, "i32", (0, 10, 33)), P, ctx.new_acc(P), 100).cpu().numpy()
    want = exp.astype(np.float64)
    err = np.abs(got - want) / np.maximum(want, 1)
    print("S2 beyond 2^53: worst relative error", err.max())
    assert (err <= 1e-12).all() and (got[:, 1:] > 0).all() and (got[:, 0] == 0).all()  # the major base is no background


# ---- omega and the planted cohort through Context ---------------------------------------------------------------------------------------

PLANTED = dict(P=200, S=32, T=4)


def _panel(ctx, normals, P, layout="u16", cuts=None):
    """thr of the whole panel (C_VALUE), its C = 0 table, dispersion's planes, S2 and omega, as the command line computes them"""
    S = normals.shape[0]
    cuts = cuts or (0, S // 2, S)
    ch = _chunks(ctx, normals, P, 0, None, None, None, layout, cuts)
    acc, acc0 = ctx.new_acc(P), ctx.new_acc(P)
    table = None
    for i, rec in enumerate(ch):
        table = ctx.error_reduce_records(rec, P, acc, C_VALUE, COV, first_sample=cuts[i], accumulate=i > 0, finalize=i == len(ch) - 1)
        ctx.error_reduce_records(rec, P, acc0, 0.0, COV, first_sample=cuts[i], accumulate=i > 0, summary=True)
    disp = ctx.panel_dispersion(ch, P, acc0, COV, Z_CUTOFF, samples=False)
    s2 = ctx.overdispersion_sums(ch, P, acc0, COV)
    omega = ctx.overdispersion_fit(P, acc0, disp["x2"], s2, disp["status"])
    return table, acc0, disp, s2, omega


def test_omega_and_the_planted_cohort(ctx):
    (normals, tumours, ref, over, variants), dm, s2_exp, _, _ = planted_and_fit(**PLANTED)
    P, T = normals.shape[1], tumours.shape[0]
    table, acc0, disp, s2, omega = _panel(ctx, normals, P)
    assert np.array_equal(s2.cpu().numpy(), s2_exp.astype(np.float64))
    status, x2 = disp["status"].cpu().numpy(), disp["x2"].cpu().numpy()
    w = omega.cpu().numpy()
    # the device's omega against the model fed the device's own X2 and status: the forward bound; a cell that is not HIGH is exactly 0
    w_exp, bound = omega_model(status, dm["n"], dm["K"], dm["D"], x2, s2_exp)
    high = (status & HIGH) != 0
    assert (w[~high] == 0).all() and high.sum() >= 2 * len(over) and all(high[0, b, p] and high[1, b, p] for p, b in over)
    print("omega: worst error over its bound", np.max(np.abs(w - w_exp)[high] / bound[high]), "of", int(high.sum()), "HIGH cells")
    assert (np.abs(w - w_exp) <= bound).all()
    # both scores of every tumour cell against the model, with the device's own table
    thr = table.thr.cpu().numpy().reshape(2, 4, P)
    rt = ctx.records(_pack(ctx, tumours, "u16"), "u16", T)
    d_ref = _t(ref)
    q0 = ctx.nb_score(rt, P, table.thr, d_ref, None, 100).cpu().numpy()
    q = ctx.nb_score(rt, P, table.thr, d_ref, omega, 100).cpu().numpy()
    q0_m, _ = score_model(tumours, P, thr, None, ref, 100)
    q_m, _ = score_model(tumours, P, thr, w, ref, 100)
    print("worst |Q - model|", np.abs(q0.astype(np.float64) - q0_m).max(), np.abs(q.astype(np.float64) - q_m).max())
    assert (np.abs(q0.astype(np.float64) - q0_m) <= Q_TOL).all() and (np.abs(q.astype(np.float64) - q_m) <= Q_TOL).all()
    assert np.array_equal(q0 == NA, q0_m == NA) and (q0 != NA).sum() == T * P * 6
    tm, tg = tally(q0_m, q_m, 13.0, over, variants), tally(q0, q, 13.0, over, variants)
    print("model ", tm)
    print("device", tg)
    assert tg["over_kept"] <= 2 * tm["over_kept"] and tg["ordinary_kept"] <= 2 * tm["ordinary_kept"] and tg["over_poisson"] <= 2 * tm["over_poisson"]
    assert all(tg["var_ordinary_kept"]) and len(tg["var_ordinary_kept"]) == 16
    assert tg["over_kept"] < tg["over_poisson"]


# ---- Q -----------------------------------------------------------------------------------------------------------------------------------

CUTOFF = 100
THR = np.array([-1.0, 0.0, 1e-6, 0.0005, 0.001, 0.002, 0.0031, 0.01, 0.05], np.float32)
OMEGA = np.array([0.0, 0.0, 0.0, 1e-8, 0.01, 0.3, 1.0, 1.5, 7.0, 1e4])
DEPTH = np.array([CUTOFF - 1, CUTOFF, CUTOFF + 1, 500, 2000, 60000])


@functools.lru_cache(maxsize=None)
def _q_case(P, n_t):
    """records, table and omega drawn from few values (the model sums every distinct tail once), with both cut-off sweeps per strand,
    reference codes 255 and 4, absent records and a few omegas that are not numbers"""
    rng = np.random.default_rng(7 * P + n_t)
    ref = rng.integers(0, 4, P).astype(np.uint8)
    ref[rng.random(P) < 0.08] = 255
    ref[rng.random(P) < 0.05] = 4
    d = DEPTH[rng.integers(0, len(DEPTH), size=(n_t, P, 2))]
    alt = rng.poisson(rng.choice([0.3, 2.0, 9.0], size=(n_t, P, 2, 4)))
    alt = np.minimum(alt, d[..., None] // 4)
    recs = np.zeros((n_t, P, 8), np.int64)
    for st in range(2):
        recs[:, :, st * 4:st * 4 + 4] = alt[:, :, st]
        major = np.where(ref < 4, ref, 0)
        recs[:, np.arange(P), st * 4 + major] = 0
        recs[:, np.arange(P), st * 4 + major] = d[:, :, st] - recs[:, :, st * 4:st * 4 + 4].sum(-1)
    recs = recs.astype(np.int32)
    gone = rng.random((n_t, P)) < 0.06
    recs[gone] = 0
    recs[gone, 0] = ABSENT
    thr = THR[rng.integers(0, len(THR), size=(2, 4, P))]
    omega = OMEGA[rng.integers(0, len(OMEGA), size=(2, 4, P))].copy()
    bad = rng.random((2, 4, P)) < 0.03
    omega[bad] = rng.choice([-1e-9, np.nan, np.inf, -np.inf], size=int(bad.sum()))
    q0, _ = score_model(recs, P, thr, None, ref, CUTOFF)
    q, q64 = score_model(recs, P, thr, omega, ref, CUTOFF)
    return recs, ref, thr, omega, q0, q, q64


@pytest.mark.parametrize("layout", ["i32", "u24", "u16"])
@pytest.mark.parametrize("P,n_t", [(1, 1), (63, 4), (64, 5), (65, 9), (130, 5)])
def test_q_equals_the_model(ctx, layout, P, n_t):
    recs, ref, thr, omega, q0_m, q_m, q64 = _q_case(P, n_t)
    rt = ctx.records(_pack(ctx, recs, layout), layout, n_t)
    d_thr, d_ref, d_w = _t(thr), _t(ref), _t(omega)
    q0 = ctx.nb_score(rt, P, d_thr, d_ref, None, CUTOFF).cpu().numpy()
    qz = ctx.nb_score(rt, P, d_thr, d_ref, _t(np.zeros((2, 4, P))), CUTOFF).cpu().numpy()
    q = ctx.nb_score(rt, P, d_thr, d_ref, d_w, CUTOFF).cpu().numpy()
    assert q0.tobytes() == qz.tobytes()  # d_omega NULL is an array of zeros
    for got, want in ((q0, q0_m), (q, q_m)):
        exact = (want == NA) | (want == np.float32(-888)) | (want == 0)
        assert np.array_equal(got[exact], want[exact]) and np.array_equal(got == NA, want == NA)
        assert (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= Q_TOL).all()
    if P >= 63:
        ev = q_m != NA
        assert (q_m == np.float32(-888)).any() and (q_m[ev] == 0).any() and (q_m == 100).any() and ((q_m > 0) & (q_m < 100)).sum() > 50
        assert (~ev).sum() > ev.sum() // 8 and (q0_m != NA).sum() > ev.sum()  # NA by record, depth and reference code; and by a bad omega
        for q_min in (5.0, 13.0, 20.0):
            band = ev & (np.abs(q64 - q_min) <= 2e-5).any(axis=-1, keepdims=True)
            assert band.sum() < 0.01 * ev.sum()
            keep = ~band.any(axis=-1)
            assert np.array_equal(decisions(q, q_min)[keep], decisions(q_m, q_min)[keep])


def test_cutoff_sweep_per_strand(ctx):
    """a strand at calling_cutoff - 1 makes the whole record NA, at the cut-off it is scored"""
    P = 4
    recs = np.zeros((1, P, 8), np.int32)
    for p, (fw, bw) in enumerate(((99, 100), (100, 99), (100, 100), (99, 99))):
        recs[0, p] = [fw - 3, 3, 0, 0, bw - 2, 2, 0, 0]
    ref = np.zeros(P, np.uint8)
    thr = np.full((2, 4, P), 0.002, np.float32)
    q = ctx.nb_score(ctx.records(_t(recs), "i32", 1), P, _t(thr), _t(ref), None, 100).cpu().numpy()
    assert (q[0, [0, 1, 3]] == NA).all() and (q[0, 2, 0] == NA).all() and (q[0, 2, 1:] != NA).all() and (q[0, 2, 1] > 0).all()
    q = ctx.nb_score(ctx.records(_t(recs), "i32", 1), P, _t(thr), _t(ref), None, 99).cpu().numpy()
    assert (q[0, :, 1:] != NA).all() and (q[0, :, 0] == NA).all()


def test_grid_corners_in_records(ctx):
    """the recorded grid's far corners (k up to 100 000, m up to 1e4, omega up to 1e4, depth 2^31 - 1) as records of one int32 row"""
    g = np.load(os.path.join(GOLDEN, "overdispersion", "nb_grid.npz"))
    k, d, e, w, want = g["k"], g["d"], g["e"], g["omega"], g["q"]
    m = d.astype(np.float64) * e.astype(np.float64)
    ok = (k <= d) & (e > 0) & (k > 0)
    pick = np.concatenate([np.nonzero(ok & (k >= 9000))[0][::4], np.nonzero(ok & (k < 9000) & ((w >= 100) | (d == 2 ** 31 - 1)))[0][::9][:100]])
    P = len(pick)
    assert P >= 120 and k[pick].max() >= 99999 and w[pick].max() == 1e4 and d[pick].max() == 2 ** 31 - 1
    recs = np.zeros((1, P, 8), np.int32)
    recs[0, :, 0] = d[pick] - k[pick]
    recs[0, :, 1] = k[pick]
    recs[0, :, 4:] = recs[0, :, :4]
    thr = np.zeros((2, 4, P), np.float32)
    omega = np.zeros((2, 4, P))
    thr[:, 1], omega[:, 1] = e[pick], w[pick]
    thr[:, 2:], omega[:, 2:] = -1.0, 0.5
    q = ctx.nb_score(ctx.records(_t(recs), "i32", 1), P, _t(thr), _t(np.zeros(P, np.uint8)), _t(omega), 0).cpu().numpy()
    err = np.abs(q[0, :, 1, :].astype(np.float64) - want[pick][:, None])
    print("corners: worst |Q - model|", err.max())
    assert (err <= Q_TOL).all() and (q[0, :, 0] == NA).all() and (q[0, :, 2:] == np.float32(-888)).all()
