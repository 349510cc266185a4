"""The host exports of the spectrum functions of csrc/ampli_math.h (ampli_host_spectrum_enters_batch / _class / _fold / _score: the text
spectrum_kernel and the command line run, compiled for the host) against the definition in tests/spectrum_model.py: the gate on 20 000
random records and on its boundary grid, the class on every argument, folds and scores of 20 000 random sum matrices in cohorts of
every kind -- integers with np.array_equal, doubles bit for bit with NaNs matched by position."""
import ctypes as C

import numpy as np

from amplisolve_amd import host_lib
from amplisolve_amd._lib import SpectrumParams
from tests.spectrum_cohorts import N_NORMALS, planted, planted_results
from tests.spectrum_model import ABSENT, CHANNELS, CLASSES, DEFAULTS, TYPES, enters, fold, same, score, spectrum_class


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _enters(recs, ref, cls, Cn, cutoff, pm):
    recs, ref, cls = np.ascontiguousarray(recs, np.int32), np.ascontiguousarray(ref, np.uint8), np.ascontiguousarray(cls, np.uint8)
    out = np.full(len(recs), 7, np.uint8)
    assert host_lib().ampli_host_spectrum_enters_batch(_p(recs), len(recs), _p(ref), _p(cls), Cn, cutoff, pm, _p(out)) == 0
    return out.astype(bool)


def test_the_gate_equals_the_model_on_random_records_and_on_its_grid():
    rng = np.random.default_rng(170)
    n = 20000
    depth = rng.choice([0, 1, 99, 100, 101, 500, 1000, 1010, 30000], (n, 2))
    recs = np.zeros((n, 8), np.int64)
    ref = rng.choice([0, 1, 2, 3, 4, 255], n, p=[0.23, 0.23, 0.23, 0.23, 0.04, 0.04]).astype(np.uint8)
    r = np.where(ref <= 3, ref, 0)
    for st in range(2):
        alts = (depth[:, st, None] * rng.choice([0.0, 0.0, 0.01, 0.015, 0.0299, 0.03, 0.0301, 0.06, 0.5], (n, 4))).astype(np.int64)
        alts[np.arange(n), r] = 0
        recs[:, 4 * st:4 * st + 4] = alts
        recs[np.arange(n), 4 * st + r] = np.maximum(depth[:, st] - alts.sum(1), 0)
    recs[rng.random(n) < 0.05] = [ABSENT, 0, 0, 0, 0, 0, 0, 0]
    top = (1 << 31) - 1
    recs[:8] = [[top] * 8, [top, 0, 0, 0, top, 0, 0, 0], [top, top // 40, 0, 0, top, 0, 0, 0], [0] * 8, [1 << 30, 1 << 25, 0, 0, 1 << 30, 0, 0, 0],
                [100, 0, 0, 0, 100, 0, 0, 0], [99, 0, 0, 0, 100, 0, 0, 0], [485, 15, 0, 0, 485, 15, 0, 0]]
    cls = rng.choice([0, 1, 17, 63, 64, 67, 68, 127, 128, 254, 255], n).astype(np.uint8)
    hits = 0
    for Cn, cutoff, pm in ((68, 100, 30), (68, 0, 30), (1, 100, 30), (128, 101, 0), (18, 1, 1000), (68, 100, 15)):
        got, exp = _enters(recs, ref, cls, Cn, cutoff, pm), enters(recs, ref, cls, Cn, cutoff, pm)
        assert np.array_equal(got, exp), np.flatnonzero(got != exp)[:5]
        hits += exp.sum()
    assert 5000 < hits < 60000
    L = host_lib()
    out = np.full(4, 7, np.uint8)
    r4, z4 = np.zeros((4, 8), np.int32), np.zeros(4, np.uint8)
    for bad in ((None, 4, _p(z4), _p(z4), 68, 100, 30, _p(out)), (_p(r4), 4, None, _p(z4), 68, 100, 30, _p(out)), (_p(r4), 4, _p(z4), None, 68, 100, 30, _p(out)),
                (_p(r4), 4, _p(z4), _p(z4), 68, 100, 30, None), (_p(r4), -1, _p(z4), _p(z4), 68, 100, 30, _p(out)), (_p(r4), 4, _p(z4), _p(z4), 0, 100, 30, _p(out)),
                (_p(r4), 4, _p(z4), _p(z4), 129, 100, 30, _p(out)), (_p(r4), 4, _p(z4), _p(z4), 68, -1, 30, _p(out)), (_p(r4), 4, _p(z4), _p(z4), 68, 100, -1, _p(out)),
                (_p(r4), 4, _p(z4), _p(z4), 68, 100, 1001, _p(out))):
        assert L.ampli_host_spectrum_enters_batch(*bad) == -1
    assert (out == 7).all()


def test_the_class_of_every_argument():
    L = host_lib()
    for r in (0, 1, 2, 3, 4, 200, 255):
        for l in (0, 1, 2, 3, 4, 255):
            for t in (0, 1, 2, 3, 4, 255):
                assert L.ampli_host_spectrum_class(r, l, t) == spectrum_class(r, l, t), (r, l, t)


def _fold(sums):
    S = sums.shape[0]
    alt, dep, sites = np.full((S, 2, TYPES), -1, np.int64), np.full((S, 2, TYPES), -1, np.int64), np.full((S, TYPES), -1, np.int64)
    ca, cd = np.full((S, CHANNELS), -1, np.int64), np.full((S, CHANNELS), -1, np.int64)
    assert host_lib().ampli_host_spectrum_fold(_p(sums), S, _p(alt), _p(dep), _p(sites), _p(ca), _p(cd)) == 0
    return dict(alt=alt, dep=dep, sites=sites, ctx_alt=ca, ctx_dep=cd)


def _score(f, n_normals, **kw):
    S = f["alt"].shape[0]
    prm = SpectrumParams(kw["min_sites"], kw["min_normals"], kw["excess_ratio"], kw["z_cutoff"], kw["asym_delta"])
    d = lambda *shape: np.full(shape, -7.0)  # noqa: E731
    out = dict(ref=d(TYPES, 4), n_eff=np.full(TYPES, -1, np.int32), status=np.full(TYPES, 9, np.uint8), rate2=d(S, TYPES), ratio=d(S, TYPES), z=d(S, TYPES),
               asym=d(S, TYPES), za=d(S, TYPES), flag=np.full((S, TYPES), 9, np.uint8))
    assert host_lib().ampli_host_spectrum_score(_p(f["alt"]), _p(f["dep"]), _p(f["sites"]), S, n_normals, C.byref(prm), _p(out["ref"]), _p(out["n_eff"]),
                                                _p(out["status"]), _p(out["rate2"]), _p(out["ratio"]), _p(out["z"]), _p(out["asym"]), _p(out["za"]),
                                                _p(out["flag"])) == 0
    return out


def _equal(got, exp):
    for k in ("alt", "dep", "sites", "ctx_alt", "ctx_dep", "n_eff", "status", "flag"):
        if k in exp:
            assert np.array_equal(got[k], exp[k]), k
    for k in ("ref", "rate2", "ratio", "z", "asym", "za"):
        if k in exp:
            assert same(got[k], exp[k]), k


def test_folds_and_scores_equal_the_model_on_random_matrices():
    rng = np.random.default_rng(171)
    PRM = {k: DEFAULTS[k] for k in ("min_sites", "min_normals", "excess_ratio", "z_cutoff", "asym_delta")}
    done, flags = 0, set()
    is_ref = np.array([[y == (c >> 4 if c < 64 else c - 64) for y in range(4)] for c in range(CLASSES)])
    kind = 0
    while done < 20000:
        S = int(rng.choice([1, 2, 5, 6, 7, 13, 40]))
        N = int(rng.integers(0, S + 1))
        kind += 1
        sums = np.zeros((S, CLASSES, 9), np.int64)
        sums[:, :, 0] = rng.integers(0, 30, (S, CLASSES)) * rng.choice([0, 1, 1, 1], (S, 1))
        depth = rng.integers(100, 5000, (S, CLASSES, 2)) * sums[:, :, 0, None]
        scale = rng.choice([1, 1, 1, 1 << 20], 1)[0]  # sums beyond 2^40 too
        lam = depth[..., None] * rng.choice([0.0, 1e-4, 1e-3, 5e-3], (S, CLASSES, 2, 4)) * rng.choice([1.0, 1.0, 4.0], (S, 1, 1, 1))
        k = np.where(is_ref[None, :, None, :], 0, rng.poisson(lam))
        k += is_ref[None, :, None, :] * (depth - k.sum(-1)).clip(0)[..., None]
        sums[:, :, 1:] = (k * scale).reshape(S, CLASSES, 8)
        if kind % 5 == 0 and S > 2:
            sums[1:N] = sums[0]  # equal normals: mad == 0
        if kind % 7 == 0:
            sums[:, :, 1:] = 0   # sites without reads: every rate is NaN
        exp = fold(sums)
        got = _fold(sums)
        _equal(got, exp)
        for prm in (PRM, dict(min_sites=1, min_normals=1, excess_ratio=1.5, z_cutoff=2.0, asym_delta=0.05)):
            es = score(exp, N, **prm)
            _equal(_score(got, N, **prm), es)
            flags |= set(es["flag"].ravel().tolist())
        done += S
    assert flags == {0, 1, 2, 3, 4}
    L = host_lib()
    z = np.zeros(4 * CLASSES * 9, np.int64)
    assert L.ampli_host_spectrum_fold(None, 1, _p(z), _p(z), _p(z), None, None) == -1 and L.ampli_host_spectrum_fold(_p(z), -1, _p(z), _p(z), _p(z), None, None) == -1
    alt = np.full((1, 2, TYPES), -1, np.int64)
    assert L.ampli_host_spectrum_fold(_p(z), 1, _p(alt), _p(z[100:]), _p(z[200:]), None, None) == 0 and not alt.any()  # without the channels


def test_the_planted_cohort_on_the_host():
    c, r = planted(), planted_results()
    assert r["sums"].shape == (18, CLASSES, 9) and c["recs"].shape[0] == 18
    got = _fold(np.ascontiguousarray(r["sums"]))
    _equal(got, r["fold"])
    prm = {k: DEFAULTS[k] for k in ("min_sites", "min_normals", "excess_ratio", "z_cutoff", "asym_delta")}
    _equal(_score(got, N_NORMALS, **prm), r["score"])
    prm = SpectrumParams(1, 1, 3.0, 10.0, 0.15)
    z = np.zeros(18 * 2 * TYPES, np.float64)
    assert host_lib().ampli_host_spectrum_score(_p(got["alt"]), _p(got["dep"]), _p(got["sites"]), 18, 19, C.byref(prm), *([_p(z)] * 9)) == -1
    assert host_lib().ampli_host_spectrum_score(_p(got["alt"]), _p(got["dep"]), _p(got["sites"]), 0, 0, C.byref(prm), *([_p(z)] * 9)) == -1
    assert host_lib().ampli_host_spectrum_score(_p(got["alt"]), None, _p(got["sites"]), 18, 12, C.byref(prm), *([_p(z)] * 9)) == -1
