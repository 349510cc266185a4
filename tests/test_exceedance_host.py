"""The host export of the candidate rule of csrc/ampli_math.h (ampli_host_exceedance_candidate_batch: the text the command line runs,
compiled for the host) against the definition in tests/exceedance_model.py, 0 / 1 with np.array_equal: 20 000 random cells with every
clause at its bound, fields of 2^31 - 1, the planted cohort, and the refusals."""
import ctypes as C

import numpy as np

from amplisolve_amd import host_lib
from amplisolve_amd._lib import ExceedanceParams
from tests.exceedance_cohorts import CAND, N_NORMALS, planted, planted_results
from tests.exceedance_model import NA, candidate_cells, counts

PRM = ("min_alt_reads", "min_vaf_pm", "min_normals", "max_normals")


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _host(x, depth, elig, ge, **prm):
    x, depth = np.ascontiguousarray(x, np.uint64).reshape(-1, 2), np.ascontiguousarray(depth, np.uint64).reshape(-1, 2)
    elig, ge = np.ascontiguousarray(elig, np.uint16).reshape(-1), np.ascontiguousarray(ge, np.uint16).reshape(-1, 2)
    out = np.full(len(elig), 7, np.uint8)
    q = ExceedanceParams(*[prm[k] for k in PRM])
    assert host_lib().ampli_host_exceedance_candidate_batch(_p(x), _p(depth), _p(elig), _p(ge), len(elig), C.byref(q), _p(out)) == 0
    assert set(out.tolist()) <= {0, 1}
    return out.astype(bool)


def test_the_rule_equals_the_model_on_random_cells_with_every_clause_at_its_bound():
    rng = np.random.default_rng(180)
    n = 20000
    top = (1 << 31) - 1
    hits = 0
    for prm in (dict(CAND), dict(min_alt_reads=0, min_vaf_pm=0, min_normals=0, max_normals=0), dict(min_alt_reads=5, min_vaf_pm=20, min_normals=24, max_normals=1),
                dict(min_alt_reads=1, min_vaf_pm=1000, min_normals=1, max_normals=65534), dict(min_alt_reads=top, min_vaf_pm=250, min_normals=65534, max_normals=65535)):
        mar, pm, mn, mx = (prm[k] for k in PRM)
        x = rng.choice([0, 1, 2, 3, 4, 5, 6, 40, max(mar - 1, 0), mar, mar + 1, top], (n, 2)).astype(np.uint64)
        depth = np.maximum(rng.choice([0, 100, 1000, 4000, 4 * top], (n, 2)).astype(np.uint64), x)
        # the fraction at its bound: 1000 (x0 + x1) == pm (d0 + d1), and one read either side
        k = rng.random(n) < 0.4
        tot = rng.integers(1, 3000, n) * 1000
        alt = tot // 1000 * pm + rng.integers(-1, 2, n)
        alt = np.clip(alt, 0, tot)
        x[k, 0], x[k, 1] = (alt // 2)[k], (alt - alt // 2)[k]
        depth[k, 0], depth[k, 1] = (tot // 2)[k], (tot - tot // 2)[k]
        elig = rng.choice([0, 1, 9, 10, 11, 23, 24, 25, max(mn - 1, 0), min(mn, 65535), min(mn + 1, 65535), 65534], n).astype(np.uint16)
        ge = rng.choice([0, 0, 0, 1, 2, max(mx - 1, 0), min(mx, 65534), min(mx + 1, 65534), 65534, NA], (n, 2), p=[0.3, 0.2, 0.1] + [0.4 / 7] * 7).astype(np.uint16)
        got, exp = _host(x, depth, elig, ge, **prm), candidate_cells(x, depth, elig, ge, **prm)
        assert np.array_equal(got, exp), np.flatnonzero(got != exp)[:5]
        hits += int(exp.sum())
        for clause in range(4 if mar < top else 0):  # every clause decides some cell on its own (the last set is about the widths)
            loose = dict(prm)
            loose[PRM[clause]] = 65535 if clause == 3 else 0
            assert loose == prm or (clause == 3 and mx >= 65534) or candidate_cells(x, depth, elig, ge, **loose).sum() > exp.sum(), (prm, clause)
    assert 500 < hits < 60000


def test_fields_of_two_to_the_thirty_one_minus_one():
    top = (1 << 31) - 1
    x = np.array([[top, top], [top, top], [top, top - 1], [1, 1]], np.uint64)
    depth = np.array([[top, top], [4 * top, 4 * top], [top, top], [4 * top, 4 * top]], np.uint64)
    elig, ge = np.full(4, 24, np.uint16), np.zeros((4, 2), np.uint16)
    for pm, exp in ((1000, [1, 0, 0, 0]), (250, [1, 1, 1, 0]), (251, [1, 0, 1, 0]), (0, [1, 1, 1, 1])):
        prm = dict(min_alt_reads=1, min_vaf_pm=pm, min_normals=24, max_normals=0)
        assert _host(x, depth, elig, ge, **prm).tolist() == [bool(v) for v in exp] == candidate_cells(x, depth, elig, ge, **prm).tolist(), pm
    assert 1000 * 2 * top < 1 << 64 and 1000 * 8 * top < 1 << 64


def test_the_planted_cohort():
    c, r = planted(), planted_results()
    recs = c["recs"][N_NORMALS:]
    _, x, D = counts(recs)
    x = np.ascontiguousarray(x.transpose(0, 1, 3, 2))
    depth = np.ascontiguousarray(np.broadcast_to(D[:, :, None, :], x.shape))
    elig = np.ascontiguousarray(np.broadcast_to(r["elig"][:, :, None], x.shape[:3]))
    got = _host(x, depth, elig, r["ge"], **CAND).reshape(x.shape[:3])
    assert np.array_equal(got, r["cand"]) and got.sum() >= 40


def test_refusals():
    L = host_lib()
    x, e, g, out = np.zeros((4, 2), np.uint64), np.zeros(4, np.uint16), np.zeros((4, 2), np.uint16), np.full(4, 7, np.uint8)
    ok = ExceedanceParams(3, 0, 10, 0)
    args = [_p(x), _p(x), _p(e), _p(g), 4, C.byref(ok), _p(out)]
    for k in (0, 1, 2, 3, 5, 6):
        bad = list(args)
        bad[k] = None
        assert L.ampli_host_exceedance_candidate_batch(*bad) == -1
    assert L.ampli_host_exceedance_candidate_batch(*(args[:4] + [-1] + args[5:])) == -1
    for q in (ExceedanceParams(-1, 0, 10, 0), ExceedanceParams(3, -1, 10, 0), ExceedanceParams(3, 1001, 10, 0), ExceedanceParams(3, 0, -1, 0),
              ExceedanceParams(3, 0, 10, -1)):
        assert L.ampli_host_exceedance_candidate_batch(*(args[:5] + [C.byref(q)] + args[6:])) == -1
    assert (out == 7).all()
    assert L.ampli_host_exceedance_candidate_batch(*(args[:4] + [0] + args[5:])) == 0 and (out == 7).all()
    assert L.ampli_host_exceedance_candidate_batch(*args) == 0 and (out == 0).all()  # no reads: below min_alt_reads
