"""ampli_loo_call_records, the leave-one-out check of the panel of normals, against the composed CPU model (tests/loo_model.py):
masks, S-1 thresholds, callable counts and the call list bit for bit, over every record layout, chunked cohorts, extra occurrences,
lines with their own RD column, S from 1 to 64 and P not a multiple of 64; both modes; the envelope flag."""
import numpy as np
import pytest

from tests.helpers import edge_case_recs, synth_recs, synth_ref
from tests.loo_model import loo_model
from tests.test_gpu_parity import _t

pytestmark = pytest.mark.gpu
ABSENT = np.iinfo(np.int32).min


def _pack(ctx, recs32, layout):
    t = _t(recs32)
    if layout == "i32":
        return t
    out, fits = ctx.pack(t, layout)
    assert fits
    return out


def _cohort(P, S, seed, extras=False, own_rd=False, u16=False):
    """synthetic normals (depth 2000) with edge-case records on a tenth of the positions and spiked low-level variants that the
    S-1 tables of the other normals call; extras: a sixth of the positions listed twice, a few three times"""
    rng = np.random.default_rng(seed)
    recs = synth_recs(P, S, seed=0xA3F15017 + seed)
    k = max(1, P // 10)
    recs[:, P - k:] = edge_case_recs(k, S, rng)
    for _ in range(max(2, P * S // 40)):  # alt reads at 0.5-30 % on both strands of one normal
        s, p, nt = int(rng.integers(S)), int(rng.integers(P - k)), int(rng.integers(4))
        if recs[s, p, 0] == ABSENT:
            continue
        frac = rng.choice([0.005, 0.01, 0.03, 0.3])
        for st in range(2):
            d = int(recs[s, p, st * 4:st * 4 + 4].sum())
            recs[s, p, st * 4 + nt] += int(d * frac)
    E, dup_off, ext_pos = 0, None, None
    if extras:
        mult = np.zeros(P, np.int64)
        mult[rng.choice(P, max(1, P // 6), replace=False)] = 1
        mult[rng.choice(P, max(1, P // 40), replace=False)] = 2
        dup_off = np.concatenate([[0], np.cumsum(mult)]).astype(np.uint32)
        E = int(dup_off[-1])
        ext_pos = np.repeat(np.arange(P), mult).astype(np.uint32)
        ext = recs[:, ext_pos].copy()  # the same amplicon region read again: close to the primary line, sometimes absent
        ext[:, :, :8] = np.where(ext[:, :, :1] == ABSENT, ext, ext + rng.integers(0, 3, ext.shape).astype(np.int32))
        gone = rng.random((S, E)) < 0.15
        ext[gone] = 0
        ext[gone, 0] = ABSENT
        recs = np.concatenate([recs, ext], axis=1)
    if u16:
        recs = np.where(recs == ABSENT, ABSENT, np.minimum(recs, 65534)).astype(np.int32)
    rd = None
    if own_rd:
        R = P + E
        rd = np.full((S, R), ABSENT, np.int32)
        pick = (rng.random((S, R)) < 0.1) & (recs[:, :, 0] != ABSENT)
        tot = recs.sum(-1)
        rd[pick] = (tot[pick] + rng.integers(0, 50, pick.sum())).astype(np.int32)
    ref_code = synth_ref(P, seed=0xA3F15017 + seed)
    ref_code[rng.choice(P, max(1, P // 50), replace=False)] = 255  # N in the reference: no record callable there
    return recs, E, dup_off, ext_pos, rd, ref_code


def _gpu(ctx, recs, P, E, dup_off, ext_pos, rd, ref_code, layout, cuts, C, cov, call_cov, mode, dense=True):
    """the whole cohort reduced chunk by chunk into one table, then one leave-one-out launch per resident chunk"""
    import torch

    S = recs.shape[0]
    acc = ctx.new_acc(P)
    chunks = []
    for ci in range(len(cuts) - 1):
        lo, hi = cuts[ci], cuts[ci + 1]
        kw = {}
        if E:
            kw.update(dup_off=_t(dup_off), ext_pos=_t(ext_pos))
        if rd is not None:
            kw.update(rd=_t(rd[lo:hi, :P]), rd_ext=_t(rd[lo:hi, P:]) if E else None)
        rec = ctx.records(_pack(ctx, recs[lo:hi], layout), layout, hi - lo, E=E, **kw)
        ctx.error_reduce_records(rec, P, acc, C, cov, first_sample=lo, accumulate=ci > 0, summary=True)
        chunks.append((lo, rec))
    callable_pos = torch.zeros((P,), dtype=torch.int32, device=ctx.device)
    flags = torch.zeros((1,), dtype=torch.int32, device=ctx.device)
    out = dict(call_mask=[], thr_loo=[], callable_sample=[], calls=[])
    for lo, rec in chunks:
        res = ctx.loo_call(rec, P, acc, _t(ref_code), C, cov, call_cov, mode=mode, capacity=4 * rec.n_samples * (P + E) + 64,
                           dense_thr=dense, callable_pos=callable_pos, flags=flags)
        out["call_mask"].append(res["call_mask"].cpu().numpy())
        if dense:
            out["thr_loo"].append(res["thr_loo"].cpu().numpy())
        out["callable_sample"].append(res["callable_sample"].cpu().numpy())
        calls = ctx.read_loo_calls(res).copy()
        calls["sample"] += lo
        out["calls"].append(calls)
    out = {k: np.concatenate(v) for k, v in out.items() if v}
    out["callable_pos"] = callable_pos.cpu().numpy()
    out["flags"] = int(flags.item())
    assert ctx.flags() & 4 == 0  # AMPLI_FLAG_QUEUE_OVERFLOW
    return out


def _check(got, exp, recs, P, rd, dense=True):
    assert np.array_equal(got["call_mask"], exp["call_mask"])
    if dense:
        assert np.array_equal(got["thr_loo"].view(np.int32), exp["thr_loo"].view(np.int32))
    assert np.array_equal(got["callable_pos"], exp["callable_pos"])
    assert np.array_equal(got["callable_sample"], exp["callable_sample"])
    calls = got["calls"]
    sure = calls[(calls["flags"] & 1) == 0]
    s_i, r_i = np.nonzero(exp["call_mask"])
    assert len(sure) == sum(bin(int(v)).count("1") for v in exp["call_mask"][s_i, r_i])
    thr = exp["thr_loo"]
    for c in calls:
        s, r, a = int(c["sample"]), int(c["record"]), int(c["alt"])
        q = exp["q"][s, r, a]
        if c["flags"] & 1:  # AMPLI_CALL_BORDERLINE: on the list either way, for the host to decide
            assert min(abs(c["q_fw"] - 5), abs(c["q_bw"] - 5)) <= 1e-6
            continue
        assert exp["call_mask"][s, r] >> a & 1
        assert abs(c["q_fw"] - q[0]) <= 1e-6 * max(1.0, abs(q[0])) and abs(c["q_bw"] - q[1]) <= 1e-6 * max(1.0, abs(q[1]))
        rec = recs[s, r]
        fw, bw = int(rec[:4].sum()), int(rec[4:].sum())
        rdv = fw + bw if rd is None or rd[s, r] == ABSENT else int(rd[s, r])
        assert (c["k_fw"], c["k_bw"], c["fw"], c["bw"], c["rd"]) == (rec[a], rec[4 + a], fw, bw, rdv)
        p = r if r < P else None
        if p is not None:
            assert (np.float32(c["thr_fw"]), np.float32(c["thr_bw"])) == (thr[s, 0, a, p], thr[s, 1, a, p])
    return len(sure)


# (P, S, chunk cuts, extras, own RD column, coverage_cutoff, calling_cutoff); an RD plane goes with the 32- and 24-bit layouts only
SHAPES = [(300, 7, (0, 7), False, False, 100, 100), (300, 7, (0, 3, 7), True, False, 30, 100), (1000, 64, (0, 20, 41, 64), True, True, 100, 30),
          (130, 2, (0, 1, 2), True, False, 1, 1), (77, 1, (0, 1), False, False, 100, 100)]
CASES = [(lay,) + sh for lay in ("i32", "u24", "u16") for sh in SHAPES if not (lay == "u16" and sh[4])]


@pytest.mark.parametrize("layout,P,S,cuts,extras,own_rd,cov,call_cov", CASES)
def test_loo_equals_the_composed_model(ctx, layout, P, S, cuts, extras, own_rd, cov, call_cov):
    from amplisolve_amd.api import POISSON_PREFILTER

    recs, E, dup_off, ext_pos, rd, ref_code = _cohort(P, S, seed=P + S, extras=extras, own_rd=own_rd, u16=layout == "u16")
    C = 0.002
    exp = loo_model(recs, P, ref_code, C, cov, call_cov, E=E, dup_off=dup_off, ext_pos=ext_pos, rd=rd)
    assert exp["order_sensitive"] == 0
    got = _gpu(ctx, recs, P, E, dup_off, ext_pos, rd, ref_code, layout, cuts, C, cov, call_cov, POISSON_PREFILTER)
    assert got["flags"] == 0
    n = _check(got, exp, recs, P, rd)
    if S > 1 and cov == 100:
        assert n > 0  # the spiked normals are called against the others' tables


@pytest.mark.parametrize("layout", ["i32", "u16"])
def test_prefilter_and_all_scores_mode_agree(ctx, layout):
    """AMPLI_POISSON_FULL queues every live pair for the drain's exact bound: the prefilter must not change a bit"""
    from amplisolve_amd.api import POISSON_FULL, POISSON_PREFILTER

    P, S = 517, 12
    recs, E, dup_off, ext_pos, rd, ref_code = _cohort(P, S, seed=3, extras=True, u16=layout == "u16")
    runs = [_gpu(ctx, recs, P, E, dup_off, ext_pos, rd, ref_code, layout, (0, 5, 12), 0.004, 100, 100, m) for m in (POISSON_PREFILTER, POISSON_FULL)]
    for k in ("call_mask", "thr_loo", "callable_pos", "callable_sample"):
        assert np.array_equal(runs[0][k], runs[1][k]), k
    exp = loo_model(recs, P, ref_code, 0.004, 100, 100, E=E, dup_off=dup_off, ext_pos=ext_pos)
    assert _check(runs[1], exp, recs, P, None) > 0


def test_without_dense_thresholds(ctx):
    """thr_loo is optional: the masks and lists do not depend on it"""
    from amplisolve_amd.api import POISSON_PREFILTER

    P, S = 640, 9
    recs, E, dup_off, ext_pos, rd, ref_code = _cohort(P, S, seed=11, extras=True)
    exp = loo_model(recs, P, ref_code, 0.002, 100, 100, E=E, dup_off=dup_off, ext_pos=ext_pos)
    got = _gpu(ctx, recs, P, E, dup_off, ext_pos, rd, ref_code, "u24", (0, 9), 0.002, 100, 100, POISSON_PREFILTER, dense=False)
    _check(got, exp, recs, P, rd, dense=False)


def test_totals_outside_the_envelope_raise_flag_bit_0(ctx):
    """deep lines at coverage_cutoff 1: the sums are no longer order-free, so the S-1 sums are not the totals minus one sample"""
    from amplisolve_amd.api import POISSON_PREFILTER

    P, S = 70, 16
    recs = synth_recs(P, S)
    recs[:, 5] = np.array([1920000, 80000, 0, 0, 1920000, 0, 80000, 0], np.int32)  # AF 4 %: every sample qualifies, 84 000 per addend
    # at coverage_cutoff 1 and C 0.002 the envelope ends at 2^20 (envelope_limit): 16 such samples are past it
    ref_code = synth_ref(P)
    got = _gpu(ctx, recs, P, 0, None, None, None, ref_code, "i32", (0, S), 0.002, 1, 100, POISSON_PREFILTER, dense=False)
    assert got["flags"] & 1
    inside = _gpu(ctx, recs, P, 0, None, None, None, ref_code, "i32", (0, S), 0.002, 100, 100, POISSON_PREFILTER, dense=False)
    assert inside["flags"] == 0
