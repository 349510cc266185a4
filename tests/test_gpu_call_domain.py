"""Every kernel poisson_call can pick, at the edges of the int32 count domain: the crafted cohort of tests/call_domain_case.py
(T = 5 x R = 137 = 685 records, int32 layout: strand depths and alt counts on both sides of AMPLI_COUNT_LIMIT = 2^24, alt counts across
the end of the lgamma table, FW = 2^31 - 2, absent records, reference code 255; thresholds 0.002 / 1e-5 / 0.25 / 0 / -1 / a negative
cell; with and without an RD column holding BW, BW - 1, 0, 2^31 - 1 and -2^30) against orc.poisson_call, with coverage cutoffs 1 and
100.  tests/test_call_domain_case.py asserts on the CPU that the case has what it is meant to have: calls, pairs the fp32 test skips,
queued-but-not-called pairs at RD >= 2^24 (the streaming kernel's `exact` test false), each arm of the drain (m > 0, m == 0, m < 0).

Routes: poisson_full_kernel (all scores, dense Q), poisson_call_kernel<FULL> (dense Q and VAFs), poisson_call_kernel<PREFILTER>
(dense VAFs), poisson_stream_kernel + the drain with the default rows per wave, 1 and 2 -- through ampli_poisson_call, and through
ampli_poisson_call_records with a row stride above P + E (the only way to an RD column: poisson_stream_kernel<I32, IRR>).

On every route, into poisoned and fenced outputs (tests/test_gpu_output_contracts.py's CallOut, tests/helpers.fenced): the mask is the
oracle's byte for byte, the list holds exactly the mask's pairs, each listed Q is within 1e-5 of the oracle's, af / af_fw / af_bw are
the oracle's bits, dense Q has the oracle's -1 / NaN pattern and lies within 1e-5, dense VAFs are the oracle's bits (a NaN for a NaN:
0 / 0 has no defined sign), no flag is raised, and no byte outside the outputs is written.

Each of the 36 cases runs the 685 records (623 present) once.  What they hold, by (cutoff, RD column) = (1, no) (1, yes) (100, no)
(100, yes): calls 297 / 174 / 263 / 154, of them with a Q = 100 168 / 126 / 168 / 118 and at RD >= 2^24 135 / 69 / 101 / 57; pairs
the stream kernel queues 1074 / 1376 / 891 / 1218 and skips in fp32 723 / 421 / 723 / 396; queued, not called, RD >= 2^24:
750 / 543 / 601 / 477; strands in the drain's arms m > 0: 755 / 546 / 674 / 487, m == 0: 0 / 57 / 0 / 49, m < 0: 46 / 586 / 39 / 519."""
import numpy as np
import pytest

from tests import call_domain_case as cd
from tests.helpers import fenced
from tests.test_gpu_output_contracts import SHARDS, CallOut, _bits
from tests.test_gpu_parity import _t

pytestmark = pytest.mark.gpu

ROUTES = ["full_q", "full_q_af", "prefilter_af", "prefilter", "prefilter_rows1", "prefilter_rows2"]
VIA = [("call", False), ("records", False), ("records", True)]  # entry point, RD column


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("via,with_rd", VIA)
@pytest.mark.parametrize("cov", [1, 100])
def test_poisson_call_at_the_edges_of_the_count_domain(ctx, cov, via, with_rd, route):
    import torch

    from amplisolve_amd.api import POISSON_FULL, POISSON_PREFILTER

    c = cd.case(cov, with_rd)
    T, P, E, R = cd.T, cd.P, cd.E, cd.R
    exp = c["exp"]
    out = CallOut(T, R, capacity=SHARDS * 3 * T * R)  # every call could land in one segment
    want_q, want_af = route in ("full_q", "full_q_af"), route in ("full_q_af", "prefilter_af")
    q, q_chk = fenced((T, R, 4, 2), torch.float64)
    af, af_chk = fenced((T, R, 4, 3), torch.float32)
    mode = POISSON_FULL if route.startswith("full") else POISSON_PREFILTER
    d_thr, d_ref, d_ext = _t(c["thr"]), _t(c["ref_code"]), _t(c["ext_pos"])
    try:
        if route.startswith("prefilter_rows"):
            ctx.set_poisson_tuning(int(route[-1]), 0)
        if via == "call":
            ctx.poisson_call(_t(c["recs"]), P, d_thr, d_ref, cov, mode=mode, E=E, ext_pos=d_ext, q=q if want_q else None,
                             af=af if want_af else None, **out.kw())
        else:
            stride = R + 9  # primaries and extras of a row in one array, rows farther apart than P + E
            rows = np.zeros((T, stride, 8), np.int32)
            rows[:, :R] = c["recs"]
            rd = c["rd"]
            rec = ctx.records(_t(rows), "i32", T, E=E, row_stride=stride, ext_pos=d_ext,
                              rd=_t(np.ascontiguousarray(rd[:, :P])) if with_rd else None,
                              rd_ext=_t(np.ascontiguousarray(rd[:, P:])) if with_rd else None)
            ctx.poisson_call_records(rec, P, d_thr, d_ref, cov, mode=mode, q=q if want_q else None, af=af if want_af else None, **out.kw())
        ctx.sync()
        assert ctx.flags() == 0
    finally:
        ctx.set_poisson_tuning()
    a = out.check(exp["call_mask"])
    q_chk()
    af_chk()
    # the list: exactly the mask's pairs (no pair of this case is near the gate: none may be flagged), the oracle's Q and VAFs
    assert len(a) == c["stats"]["calls"] and not (a["flags"] & 1).any()
    qo, afo = exp["q"][a["sample"], a["record"], a["alt"]], exp["af"][a["sample"], a["record"], a["alt"]]
    assert np.max(np.abs(a["q_fw"] - qo[:, 0])) <= 1e-5 and np.max(np.abs(a["q_bw"] - qo[:, 1])) <= 1e-5
    assert (a["q_fw"] == 100).any() or (a["q_bw"] == 100).any()
    for j, name in enumerate(("af", "af_fw", "af_bw")):
        assert np.array_equal(_bits(a[name]), _bits(afo[:, j])), name
    recs = c["recs"][a["sample"], a["record"]].astype(np.int64)
    assert np.array_equal(a["k_fw"], recs[np.arange(len(a)), a["alt"]]) and np.array_equal(a["k_bw"], recs[np.arange(len(a)), 4 + a["alt"]])
    assert np.array_equal(a["fw"], recs[:, :4].sum(-1)) and np.array_equal(a["bw"], recs[:, 4:].sum(-1))
    if want_q:
        got, want = q.cpu().numpy(), exp["q"]
        poison = _bits(got) == np.uint64(0xFFFFFFFFFFFFFFFF)
        assert not poison.any(), f"{int(poison.sum())} element(s) of q never written"
        assert np.array_equal(got == -1, want == -1) and np.array_equal(np.isnan(got), np.isnan(want))
        fin = ~np.isnan(want)
        assert np.max(np.abs(got[fin] - want[fin])) <= 1e-5
    else:
        assert bool((_bits(q.cpu().numpy()) == np.uint64(0xFFFFFFFFFFFFFFFF)).all())  # not an output of this call
    if want_af:
        got, want = af.cpu().numpy(), exp["af"]
        same = (_bits(got) == _bits(want)) | (np.isnan(got) & np.isnan(want))
        assert same.all(), (int((~same).sum()), np.argwhere(~same)[0], got[~same][:3], want[~same][:3])
    else:
        assert bool((_bits(af.cpu().numpy()) == np.uint32(0xFFFFFFFF)).all())
