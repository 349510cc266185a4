"""ampli_limit_records (Context.detection_limits) against the literal model (tests/limit_model.py): minimum reads, status, called bit
and counters of EVERY cell once the cells the device leaves open (RECHECK) are settled by ampli_host_limit_reads -- over the three
record layouts, chunks with extra occurrences, lines with their own RD column (RD - BW <= 0 among them), absent records, reference N,
thresholds -1 / 0 / the 0.01 default, coverage cut-offs 1 and 100, depths from 20 to the layout's maximum, 1 / 7 / 64 samples and
0 / 3 / 8 levels.  The called bit equals poisson_call's mask.  The device may leave at most 1 % of the searched pairs open."""
import ctypes as C

import numpy as np
import pytest

from tests import limit_model as lm
from tests.helpers import edge_case_recs, synth_recs, synth_ref
from tests.test_gpu_parity import _t

pytestmark = pytest.mark.gpu
ABSENT = np.iinfo(np.int32).min
LAYOUT_MAX = {"u16": 65534, "u24": 0xFFFFFE, "i32": (1 << 28) - 1}  # i32: four such counts per strand still sum inside int32
LEVELS = (0.001, 0.0025, 0.005, 0.01, 0.02, 0.05, 0.1, 1.0)


def _pack(ctx, recs32, layout):
    t = _t(recs32)
    if layout == "i32":
        return t
    out, fits = ctx.pack(t, layout)
    assert fits
    return out


def _inputs(layout, T, P, seed, extras, own_rd, deep):
    rng = np.random.default_rng(seed)
    recs = synth_recs(P, T, seed=0xA3F15017 + seed, depth=int(rng.choice([400, 2000, 6000])), tumour=True)
    k = max(4, P // 8)
    recs[:, P - k:] = edge_case_recs(k, T, rng)  # absent cells, depth 0 / 1 / 50 / around 100 / 33395, AF from 0 to 1
    recs[:, 0] = np.array([11, 1, 0, 0, 9, 0, 1, 0], np.int32)  # depth 20
    for _ in range(max(3, P * T // 30)):  # alternative reads at 0.2-30 % on both strands: pairs on either side of their limit
        s, p, nt = int(rng.integers(T)), int(rng.integers(1, P - k)), int(rng.integers(4))
        if recs[s, p, 0] == ABSENT:
            continue
        frac = rng.choice([0.002, 0.004, 0.006, 0.01, 0.03, 0.3])
        for st in range(2):
            recs[s, p, st * 4 + nt] += int(int(recs[s, p, st * 4:st * 4 + 4].sum()) * frac)
    if deep:  # counts at the layout's maximum
        top = LAYOUT_MAX[layout]
        for j in range(1, 4):
            recs[:, j] = np.array([top, top // 40, 7, 0, top - j, 0, top // 50, 3], np.int32)
    recs = np.where(recs == ABSENT, ABSENT, np.minimum(recs, LAYOUT_MAX[layout])).astype(np.int32)
    E, ext_pos = 0, None
    if extras:
        mult = np.zeros(P, np.int64)
        mult[rng.choice(P, max(1, P // 6), replace=False)] = 1
        mult[rng.choice(P, max(1, P // 40), replace=False)] = 2
        ext_pos = np.repeat(np.arange(P), mult).astype(np.uint32)
        E = len(ext_pos)
        ext = recs[:, ext_pos].copy()
        ext[:, :, :8] = np.where(ext[:, :, :1] == ABSENT, ext, ext + rng.integers(0, 3, ext.shape).astype(np.int32))
        gone = rng.random((T, E)) < 0.15
        ext[gone] = 0
        ext[gone, 0] = ABSENT
        recs = np.concatenate([recs, ext], axis=1)
        recs = np.where(recs == ABSENT, ABSENT, np.minimum(recs, LAYOUT_MAX[layout])).astype(np.int32)
    R = P + E
    rd = None
    if own_rd:
        rd = np.full((T, R), ABSENT, np.int32)
        present = recs[:, :, 0] != ABSENT
        tot = recs.astype(np.int64).sum(-1)
        bw = recs[:, :, 4:].astype(np.int64).sum(-1)
        pick = (rng.random((T, R)) < 0.1) & present
        rd[pick] = (tot[pick] + rng.integers(1, 50, pick.sum())).astype(np.int32)
        low = (rng.random((T, R)) < 0.03) & present  # RD - BW <= 0: no forward depth at all
        rd[low] = (bw[low] - rng.integers(0, 3, low.sum())).astype(np.int32)
    ref_code = synth_ref(P, seed=0xA3F15017 + seed)
    ref_code[rng.choice(P, max(1, P // 40), replace=False)] = 255  # N in the reference
    # thresholds as the table reader hands them over: rates rounded as "%f" text, the 0.01 default, 0 and -1
    thr = np.array([float(f"{x:f}") for x in np.exp(rng.uniform(np.log(2e-4), np.log(0.02), 8 * P))], np.float32).reshape(2, 4, P)
    kind = rng.random((2, 4, P))
    thr[kind < 0.25] = np.float32(0.01)
    thr[(kind >= 0.25) & (kind < 0.30)] = 0
    thr[(kind >= 0.30) & (kind < 0.33)] = -1
    thr[(kind >= 0.33) & (kind < 0.36)] = np.float32(1.5)  # a table from elsewhere: a mean above the strand's reads -> UNREACHABLE
    return recs, E, ext_pos, rd, ref_code, thr


def _device(ctx, recs, P, E, ext_pos, rd, ref_code, thr, layout, cuts, cov, levels):
    """one detection_limits call and one poisson_call per chunk; numpy arrays over the whole cohort"""
    from amplisolve_amd.api import POISSON_PREFILTER

    out = dict(min_reads=[], status=[], counts=[], mask=[])
    d_thr, d_ref = _t(thr), _t(ref_code)
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        kw = {}
        if E:
            kw.update(ext_pos=_t(ext_pos))
        if rd is not None:
            kw.update(rd=_t(rd[lo:hi, :P]), rd_ext=_t(rd[lo:hi, P:]) if E else None)
        rec = ctx.records(_pack(ctx, recs[lo:hi], layout), layout, hi - lo, E=E, **kw)
        res = ctx.detection_limits(rec, P, d_thr, d_ref, cov, levels)
        call = ctx.poisson_call_records(rec, P, d_thr, d_ref, cov, mode=POISSON_PREFILTER)
        for k in ("min_reads", "status", "counts"):
            out[k].append(res[k].cpu().numpy())
        out["mask"].append(call["call_mask"].cpu().numpy())
    assert ctx.flags() & 4 == 0  # AMPLI_FLAG_QUEUE_OVERFLOW
    return {k: np.concatenate(v) for k, v in out.items()}


def _compare(got, exp, recs, P, E, ext_pos, rd, ref_code, thr, cov, levels):
    searched = int(((exp["status"] & 7 == lm.OK) | (exp["status"] & 7 == lm.UNREACHABLE)).sum())
    n_open = lm.settle(got, recs, P, thr, ref_code, cov, E=E, ext_pos=ext_pos, rd=rd, levels=levels)
    assert n_open <= 0.01 * max(searched, 100), (n_open, searched)  # every strand mean of these inputs is positive and finite
    assert np.array_equal(got["status"], exp["status"])
    assert np.array_equal(got["min_reads"], exp["min_reads"])
    assert np.array_equal(got["counts"], exp["counts"])
    called = (got["status"] & lm.CALLED) != 0
    mask = (got["mask"][:, :, None] >> np.arange(4)[None, None, :]) & 1
    assert np.array_equal(called, mask.astype(bool))  # poisson_call's own mask on the same inputs
    return n_open


# (T, P, chunk cuts, extras, own RD column, coverage_cutoff, levels, counts at the layout's maximum, model scans from k = 1)
SHAPES = [(7, 150, (0, 7), False, False, 100, 3, False, True), (1, 333, (0, 1), True, True, 1, 0, True, False),
          (7, 260, (0, 3, 7), True, True, 100, 8, True, False), (64, 200, (0, 20, 41, 64), True, False, 100, 3, False, False),
          (7, 90, (0, 4, 7), True, True, 1, 8, False, True)]
CASES = [(lay,) + sh for lay in ("u16", "u24", "i32") for sh in SHAPES]


@pytest.mark.parametrize("layout,T,P,cuts,extras,own_rd,cov,n_levels,deep,from_one", CASES)
def test_limits_equal_the_model(ctx, layout, T, P, cuts, extras, own_rd, cov, n_levels, deep, from_one):
    levels = LEVELS[:n_levels]
    recs, E, ext_pos, rd, ref_code, thr = _inputs(layout, T, P, seed=P + T, extras=extras, own_rd=own_rd, deep=deep)
    exp = lm.limit_model(recs, P, thr, ref_code, cov, E=E, ext_pos=ext_pos, rd=rd, levels=levels, from_one=from_one)
    got = _device(ctx, recs, P, E, ext_pos, rd, ref_code, thr, layout, cuts, cov, levels)
    _compare(got, exp, recs, P, E, ext_pos, rd, ref_code, thr, cov, levels)
    have = set(np.unique(exp["status"] & 7).tolist())
    want = {lm.OK, lm.REF, lm.NOREF, lm.NOESTIMATE, lm.UNREACHABLE, lm.ABSENT_CODE} | ({lm.LOWDEPTH} if cov == 100 else set())
    if T > 1:
        assert want <= have, (want, have)  # every status occurs, so the cases that scan from k = 1 cover each per layout
        assert ((exp["status"] & lm.CALLED) != 0).sum() > 0 and (exp["counts"][:, 1] > 0).all()
    if n_levels:
        c = exp["counts"][:, lm.COUNTERS:]
        assert (np.diff(c, axis=1) >= 0).all() and (c[:, -1] <= exp["counts"][:, 1]).all() and c.sum() > 0


def test_counts_are_added_to_and_stats_count_evaluations(ctx):
    import torch

    P, T = 128, 3
    recs, E, ext_pos, rd, ref_code, thr = _inputs("u16", T, P, seed=5, extras=False, own_rd=False, deep=False)
    rec = ctx.records(_pack(ctx, recs, "u16"), "u16", T)
    ctx.limit_stats(reset=True)
    first = ctx.detection_limits(rec, P, _t(thr), _t(ref_code), 100, LEVELS[:2])
    once = first["counts"].cpu().numpy().copy()
    second = ctx.detection_limits(rec, P, _t(thr), _t(ref_code), 100, LEVELS[:2], counts=first["counts"])
    assert np.array_equal(second["counts"].cpu().numpy(), 2 * once)
    strands, evals, worst = ctx.limit_stats()
    exp = lm.limit_model(recs, P, thr, ref_code, 100, levels=LEVELS[:2], from_one=False)
    n_ok = int((exp["status"] & 7 == lm.OK).sum())
    assert 2 * 2 * n_ok <= strands <= 2 * 2 * (n_ok + int((exp["status"] & 7 == lm.UNREACHABLE).sum()) + int(once[:, 5].sum()))
    assert strands <= evals <= 128 * strands and 1 <= worst <= 128
    del torch


def test_bad_arguments_are_refused_before_launch(ctx):
    import torch

    P, T = 64, 2
    recs = np.minimum(synth_recs(P, T, tumour=True), 65534).astype(np.int32)
    packed = _pack(ctx, recs, "u16")
    rec = ctx.records(packed, "u16", T)
    d = ctx.device
    thr = torch.full((2, 4, P), 0.01, dtype=torch.float32, device=d)
    ref = torch.zeros((P,), dtype=torch.uint8, device=d)
    lv = torch.tensor(LEVELS, dtype=torch.float32, device=d)
    mr = torch.zeros((T, P, 4, 2), dtype=torch.int32, device=d)
    st = torch.full((T, P, 4), 0xEE, dtype=torch.uint8, device=d)
    cn = torch.zeros((T, 6 + 8), dtype=torch.int64, device=d)

    def call(rec_=rec, P_=P, thr_=thr.data_ptr(), ref_=ref.data_ptr(), cov=100, lv_=lv.data_ptr(), n=8, mr_=mr.data_ptr(), st_=st.data_ptr(),
             cn_=cn.data_ptr()):
        return ctx.lib.ampli_limit_records(ctx.h, C.byref(rec_) if rec_ is not None else None, P_, thr_, ref_, cov, lv_, n, mr_, st_, cn_)

    assert call() == 0
    torch.cuda.synchronize()
    assert (st.cpu().numpy() != 0xEE).all()
    st.fill_(0xEE)
    odd = ctx.records(packed.view(torch.uint8).flatten()[8:8 + (T * P - 1) * 16], "u16", 1)
    ext_without_index = ctx.records(packed, "u16", T, E=3)
    for bad in (dict(rec_=None), dict(P_=0), dict(thr_=None), dict(ref_=None), dict(cov=0), dict(n=9), dict(n=-1), dict(lv_=None), dict(mr_=None),
                dict(st_=None), dict(cn_=None), dict(mr_=mr.data_ptr() + 4), dict(cn_=cn.data_ptr() + 4), dict(rec_=odd),
                dict(rec_=ext_without_index, P_=P - 3)):
        rc = call(**bad)
        assert rc < 0, bad
        assert ctx.lib.ampli_last_error(ctx.h).decode() != ""
    torch.cuda.synchronize()
    assert (st.cpu().numpy() == 0xEE).all()  # nothing was launched
    assert call(lv_=None, n=0) == 0  # no levels: no level pointer needed
