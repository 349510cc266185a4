"""ampli_power_records (Context.detection_power) against the code it shares with the host (ampli_host_power_pair, every cell) and against
the pure-Python definition (tests/power_model.py, a seeded sample) -- over the three record layouts, chunks with extra occurrences,
counts at each layout's maximum, 0 / 3 / 8 levels, confidences 0.5 / 0.95 / 0.99 and either output left out.

The kernel takes whatever minimum reads it is given, so the test places them: the records are those of tests/test_gpu_limits.py, the
statuses the limit model's (plus cells still marked RECHECK), and every OK cell gets a pair of one of six kinds -- one read; every
read of the strand; round(reads x level) and its neighbours; that moved by three standard deviations; far beyond the Chernoff cut on
either side; the model's own limits.

Against the model: the power of EVERY OK cell is computed (the counters' band needs it), and power and LoD are compared on a seeded
sample of 2000 OK cells per case -- the issue's "at least 2000" met with exactly 2000 -- or on all of them where a case has fewer (the
(1, 64) shapes have under 200 OK cells, the (3, 130) shapes about 1000).  The sample always holds a cell of each of the six kinds.  Of
the rows with more than 2^20 reads, where the model's LoD sums up to 10^5 terms per tail in Python, four cells enter the sample; the
host comparison, which runs the kernel's own code compiled for the CPU and is itself pinned to the model up to 2^30 in
tests/test_power_host.py, covers every cell."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

from tests import limit_model as lm
from tests import power_model as pm
from tests.test_gpu_limits import LEVELS, _inputs, _pack
from tests.test_gpu_parity import _t

pytestmark = pytest.mark.gpu
TAIL_TOL, LOD_TOL, BAND = 1e-6, 1e-4, 2e-6
N_KINDS = 6


@functools.lru_cache(maxsize=None)
def _cohort(layout, T, P, extras, deep):
    recs, E, ext_pos, rd, ref_code, thr = _inputs(layout, T, P, seed=P + T, extras=extras, own_rd=False, deep=deep)
    exp = lm.limit_model(recs, P, thr, ref_code, 100, E=E, ext_pos=ext_pos, rd=None, levels=(), from_one=False)
    return recs, E, exp["status"], exp["min_reads"]


def _place(recs, status, min_reads, levels, seed):
    """the pairs of the OK cells by kind, a few cells back to RECHECK; returns (status, min_reads, kind [n][R][4], -1 where not OK)"""
    rng = np.random.default_rng(seed)
    status, min_reads = status.copy(), min_reads.copy()
    FW, BW = recs[:, :, :4].astype(np.int64).sum(-1), recs[:, :, 4:].astype(np.int64).sum(-1)
    kind = np.full(status.shape, -1, np.int64)
    lv = [float(np.float32(x)) for x in (levels or LEVELS)]
    for s, r, nt in np.argwhere((status & 7) == lm.OK):
        if rng.random() < 0.02:
            status[s, r, nt], min_reads[s, r, nt] = lm.RECHECK, (0, 0)
            continue
        kd = int(rng.integers(N_KINDS))
        kind[s, r, nt] = kd
        v = lv[int(rng.integers(len(lv)))]
        pair = []
        for n in (int(FW[s, r]), int(BW[s, r])):
            sd = math.sqrt(max(n * v * (1 - v), 1.0))
            k = {0: 1, 1: n, 2: round(n * v) + int(rng.integers(-1, 2)), 3: round(n * v) + int(rng.choice([-1, 1])) * round(3 * sd),
                 4: round(n * v) + int(rng.choice([-1, 1])) * (round(9 * sd) + 3), 5: 0}[kd]
            pair.append(int(np.clip(k, 1, n)))
        if kd != 5:
            min_reads[s, r, nt] = pair
    return status, min_reads, kind


def _host(FW, kf, BW, kb, levels, c):
    from amplisolve_amd import host_lib

    lv = (C.c_float * 8)(*levels)
    pw = (C.c_double * 8)()
    lod = C.c_double(0)
    assert host_lib().ampli_host_power_pair(FW, kf, BW, kb, lv, len(levels), c, pw, C.byref(lod), None) == 0
    return list(pw)[:len(levels)], lod.value


def _device(ctx, recs, P, E, status, min_reads, layout, cuts, levels, c, want_power=True, want_lod=True):
    out = dict(power=[], lod=[], counts=[])
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        rec = ctx.records(_pack(ctx, recs[lo:hi], layout), layout, hi - lo, E=E)
        res = ctx.detection_power(rec, P, _t(min_reads[lo:hi]), _t(status[lo:hi]), levels, c, want_power=want_power, want_lod=want_lod)
        for k in out:
            out[k].append(None if res[k] is None else res[k].cpu().numpy())
    return {k: None if v[0] is None else np.concatenate(v) for k, v in out.items()}


# (layout, T, P, chunk cuts, extras, counts at the layout's maximum, levels, confidence, power wanted, LoD wanted)
CASES = [("u16", 1, 64, (0, 1), False, False, 3, 0.95, True, True), ("u24", 1, 64, (0, 1), True, True, 0, 0.5, True, True),
         ("i32", 1, 64, (0, 1), False, True, 8, 0.99, True, True), ("u16", 7, 200, (0, 3, 7), True, True, 8, 0.95, True, True),
         ("u24", 7, 200, (0, 3, 7), False, True, 3, 0.99, True, True), ("i32", 7, 200, (0, 3, 7), True, False, 3, 0.5, True, True),
         ("u16", 3, 130, (0, 3), False, False, 8, 0.5, False, True), ("u24", 3, 130, (0, 3), True, False, 3, 0.95, True, False),
         ("i32", 3, 130, (0, 3), True, True, 8, 0.99, True, True)]


@pytest.mark.parametrize("layout,T,P,cuts,extras,deep,n_levels,c,want_power,want_lod", CASES)
def test_power_and_lod_equal_the_host_and_the_model(ctx, layout, T, P, cuts, extras, deep, n_levels, c, want_power, want_lod):
    levels = LEVELS[:n_levels]
    c32 = float(np.float32(c))
    recs, E, status0, min_reads0 = _cohort(layout, T, P, extras, deep)
    status, min_reads, kind = _place(recs, status0, min_reads0, levels, seed=1000 * P + T)
    got = _device(ctx, recs, P, E, status, min_reads, layout, cuts, levels, c, want_power, want_lod)
    FW, BW = recs[:, :, :4].astype(np.int64).sum(-1), recs[:, :, 4:].astype(np.int64).sum(-1)
    ok = pm.is_ok(status, min_reads, FW, BW)
    assert np.array_equal(ok, kind >= 0) and ok.sum() > 60 and (status == lm.RECHECK).sum() > 0
    assert set(np.unique(kind[ok]).tolist()) == set(range(N_KINDS))
    assert set(np.unique(status[~ok] & 7).tolist()) >= {lm.REF, lm.NOREF, lm.LOWDEPTH, lm.NOESTIMATE, lm.ABSENT_CODE}
    # every cell that is not OK: exactly 0
    if want_power:
        assert got["power"].shape == status.shape + (n_levels,) and (got["power"][~ok] == 0).all()
    if want_lod:
        assert got["lod"].shape == status.shape and (got["lod"][~ok] == 0).all()
    # every OK cell against the host's run of the same code
    cells = [tuple(x) for x in np.argwhere(ok)]
    args = {cell: (int(FW[cell[:2]]), int(min_reads[cell][0]), int(BW[cell[:2]]), int(min_reads[cell][1])) for cell in cells}
    worst_p = worst_l = 0.0
    for cell in cells:
        pw, lod = _host(*args[cell], levels, c)
        if want_power and n_levels:
            worst_p = max(worst_p, float(np.abs(got["power"][cell] - np.array(pw)).max()))
        if want_lod:
            assert 0 < got["lod"][cell] <= 1
            worst_l = max(worst_l, abs(float(got["lod"][cell]) / lod - 1))
    print(f"against the host on {len(cells)} cells: power {worst_p:.3g}, LoD {worst_l:.3g} relative")
    assert worst_p <= TAIL_TOL and worst_l <= LOD_TOL
    # the model on a seeded sample that holds every kind; of the deepest rows (the model sums every term in Python) four cells
    rng = np.random.default_rng(P + 31 * T)
    slow = [cell for cell in cells if max(args[cell][0], args[cell][2]) > 1 << 20]
    fast = [cell for cell in cells if max(args[cell][0], args[cell][2]) <= 1 << 20]
    order = [fast[i] for i in rng.permutation(len(fast))]
    first = [next(cell for cell in order if kind[cell] == kd) for kd in range(N_KINDS)]
    sample = first + [slow[i] for i in rng.permutation(len(slow))[:4]] + [cell for cell in order if cell not in first]
    sample = sample[:2000]
    assert len(sample) == min(2000, len(fast) + min(4, len(slow)))
    model_p = {cell: pm.powers(*args[cell], levels) for cell in (cells if n_levels else [])}  # all of them: the counters' band needs them
    worst_p = worst_l = 0.0
    for cell in sample:
        if want_power and n_levels:
            worst_p = max(worst_p, float(np.abs(got["power"][cell] - np.array(model_p[cell])).max()))
        if want_lod:
            worst_l = max(worst_l, abs(float(got["lod"][cell]) / pm.lod(*args[cell], c32) - 1))
    print(f"against the model on {len(sample)} cells: power {worst_p:.3g}, LoD {worst_l:.3g} relative")
    assert worst_p <= TAIL_TOL and worst_l <= LOD_TOL
    # counters
    assert np.array_equal(got["counts"][:, 0], ok.sum(axis=(1, 2)))
    if n_levels:
        mp_ = np.zeros(status.shape + (n_levels,))
        for cell in cells:
            mp_[cell] = model_p[cell]
        okx = ok[..., None]
        lo = (okx & (mp_ >= c32 + BAND)).sum(axis=(1, 2))
        hi = (okx & (mp_ >= c32 - BAND)).sum(axis=(1, 2))
        assert (hi - lo).sum() <= 0.01 * ok.sum(), (hi - lo)  # under the model alone the band is all but empty
        assert (lo <= got["counts"][:, 1:]).all() and (got["counts"][:, 1:] <= hi).all(), (lo, got["counts"], hi)
        assert (lo < ok.sum(axis=(1, 2))[:, None]).any()
        if n_levels == 8:  # the level 1.0 is among them: every OK pair passes there, and the counters are not all zero
            assert np.array_equal(got["counts"][:, 8], got["counts"][:, 0]) and lo[:, :7].sum() > 0


def test_counts_are_added_to_and_stats_count_the_work(ctx):
    layout, T, P = "u16", 3, 130
    recs, E, status0, min_reads0 = _cohort(layout, T, P, False, False)
    status, min_reads, kind = _place(recs, status0, min_reads0, LEVELS[:3], seed=7)
    rec = ctx.records(_pack(ctx, recs, layout), layout, T)
    ctx.power_stats(reset=True)
    assert ctx.power_stats() == (0, 0, 0)
    first = ctx.detection_power(rec, P, _t(min_reads), _t(status), LEVELS[:3], 0.95)
    once = first["counts"].cpu().numpy().copy()
    tails, terms, most = ctx.power_stats()
    n_ok = int((kind >= 0).sum())
    assert once[:, 0].sum() == n_ok
    assert tails >= 2 * (3 + 1) * n_ok and tails % 2 == 0  # two per level and at least one step of the search
    assert tails <= 2 * (3 + 96) * n_ok and tails <= terms and 1 <= most <= 8 * math.sqrt(65534 * 4 / 4) + 64
    second = ctx.detection_power(rec, P, _t(min_reads), _t(status), LEVELS[:3], 0.95, counts=first["counts"])
    assert np.array_equal(second["counts"].cpu().numpy(), 2 * once)
    assert ctx.power_stats(reset=True)[0] == 2 * tails and ctx.power_stats() == (0, 0, 0)


def test_bad_arguments_are_refused_before_launch(ctx):
    import torch

    P, T = 64, 2
    recs, E, status0, min_reads0 = _cohort("u16", 1, 64, False, False)
    recs = np.concatenate([recs, recs])
    status, min_reads = np.concatenate([status0, status0]), np.concatenate([min_reads0, min_reads0])
    rec = ctx.records(_pack(ctx, recs, "u16"), "u16", T)
    d = ctx.device
    mr, st = _t(min_reads), _t(status)
    lv = torch.tensor(LEVELS, dtype=torch.float32, device=d)
    pw = torch.full((T, P, 4, 8), -1.0, dtype=torch.float32, device=d)
    lod = torch.full((T, P, 4), -1.0, dtype=torch.float32, device=d)
    cn = torch.zeros((T, 9), dtype=torch.int64, device=d)

    def call(rec_=rec, P_=P, mr_=mr.data_ptr(), st_=st.data_ptr(), lv_=lv.data_ptr(), n=8, c=0.95, pw_=pw.data_ptr(), lod_=lod.data_ptr(), cn_=cn.data_ptr()):
        return ctx.lib.ampli_power_records(ctx.h, C.byref(rec_) if rec_ is not None else None, P_, mr_, st_, lv_, n, c, pw_, lod_, cn_)

    for bad in (dict(n=9), dict(c=0.4), dict(c=0.995), dict(rec_=None), dict(n=-1), dict(c=float("nan")), dict(P_=0), dict(mr_=None), dict(st_=None),
                dict(cn_=None), dict(lv_=None)):
        assert call(**bad) == -1, bad  # AMPLI_E_INVALID
        assert "bad argument" in ctx.lib.ampli_last_error(ctx.h).decode(), bad
    assert call(mr_=mr.data_ptr() + 4) == -1 and call(cn_=cn.data_ptr() + 4) == -1
    torch.cuda.synchronize()
    assert (pw.cpu().numpy() == -1).all() and (lod.cpu().numpy() == -1).all() and (cn.cpu().numpy() == 0).all()  # nothing was launched
    assert call() == 0 and call(lv_=None, n=0, pw_=None) == 0 and call(lod_=None) == 0
    torch.cuda.synchronize()
    assert (pw.cpu().numpy() >= 0).all() and (lod.cpu().numpy() >= 0).all()
