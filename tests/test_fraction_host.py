"""The host library's tumour-fraction exports (ampli_host_fraction*: csrc/ampli_math.h's text, the text the kernel runs) against the
model (tests/fraction_model.py) without a GPU: the four doubles bit for bit (== on their integer views) -- the host runs the model's
operations in the model's order --, the counts exactly, the verdict and change arithmetic, and the struct's layout against the compiler."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from amplisolve_amd import build, host_lib
from amplisolve_amd._lib import CONSTANTS, FractionParams
from tests import fraction_model as fm
from tests.fraction_cases import (COV, LIST_BAD_W, LIST_BEYOND, LIST_FULL, LIST_QUIET, LIST_REAL, LIST_SILENT, LIST_TWICE, P, ROWS, cohort, expected, lists,
                                  panel)
from tests.monitor_cases import big_records


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def host_fraction(recs, P_, thr, ref, off, cell, w, cov=COV, vaf=1000, z2=fm.Z2_95, stride=0, W=None, L=None):
    n = recs.shape[0]
    L = len(off) - 1 if L is None else L
    recs = np.ascontiguousarray(recs, np.int32)
    cell = np.ascontiguousarray(cell if len(cell) else np.zeros(1), np.uint32)
    w_ = np.ascontiguousarray(w if len(w) else np.zeros(1), np.float32)
    est, count = np.full((n, max(L, 0), 4), np.nan), np.full((n, max(L, 0), 2), -7, np.int64)
    rc = host_lib().ampli_host_fraction(_p(recs), n, stride, P_, _p(np.ascontiguousarray(thr)), _p(np.ascontiguousarray(ref)),
                                        _p(np.ascontiguousarray(off, np.uint32)), _p(cell), _p(w_), L, len(w) if W is None else W,
                                        C.byref(FractionParams(cov, vaf, z2)), _p(est), _p(count))
    return rc, est, count


def same(got, exp):
    return np.array_equal(bits(got[0]), bits(exp[0])) and np.array_equal(got[1], exp[1])


@pytest.mark.parametrize("n", ROWS)
def test_the_host_equals_the_model_bit_for_bit(n):
    thr, ref = panel()
    off, cell, w = lists()
    exp = expected(n)
    rc, est, count = host_fraction(cohort(n), P, thr, ref, off, cell, w)
    assert rc == 0 and same((est, count), exp)


def test_the_cases_hold_what_they_are_meant_to_hold():
    """every branch of the definition is taken by some (row, list) of the shared cases"""
    est, count = expected(17)
    assert (est[:, 0] == fm.NA).all() and (count[:, 0] == 0).all()                       # the empty list
    assert (est[:, LIST_BEYOND] == fm.NA).all() and (count[:, LIST_BEYOND] == 0).all()   # entries with p >= P only
    assert (count[:, LIST_TWICE, fm.N_EVAL] == 2).any() and set(count[:, LIST_TWICE, fm.N_EVAL]) <= {0, 2}
    assert (count[:, LIST_BAD_W, fm.N_EVAL] <= 2).all() and (count[:, LIST_BAD_W, fm.N_EVAL] == 2).any()  # only the two good weights count
    q = est[:, LIST_QUIET]
    assert (q[:, fm.F_HAT] == 0).all() and (q[:, fm.F_LO] == 0).all() and (q[:, fm.F_HI] > 0).all() and (q[:, fm.F_HI] < 1).all() and (q[:, fm.T0] < 0).all()
    f = est[:, LIST_FULL]
    assert (f[:, fm.F_HAT] == 1).all() and (f[:, fm.F_HI] == 1).all() and (f[:, fm.F_LO] > 0).all() and (count[:, LIST_FULL, fm.N_EVAL] == 3).all()
    s = est[:, LIST_SILENT]
    assert (s[:, fm.F_HAT] == 0).all() and (s[:, fm.F_HI] == 0).all() and (-s[:, fm.T0] >= fm.Z2_95).all()
    r = est[:, LIST_REAL]
    inner = (r[:, fm.F_HAT] > 0) & (r[:, fm.F_HAT] < 1)
    assert inner.sum() >= 8 and (r[inner, fm.F_LO] > 0).any() and (r[:, fm.F_LO] == 0).any() and (r[inner, fm.F_HI] < 1).all()
    assert (r[inner, fm.F_LO] <= r[inner, fm.F_HAT]).all() and (r[inner, fm.F_HAT] <= r[inner, fm.F_HI]).all()
    assert (count[:, :, fm.N_SEEN] < count[:, :, fm.N_EVAL]).any()
    live = est[:, :, fm.F_HAT] != fm.NA
    assert ((est[live] >= 0) | (np.arange(4) == fm.T0)).all() and (est[live][:, :3] <= 1).all()


@pytest.mark.parametrize("kw", [dict(vaf=250), dict(vaf=0), dict(cov=0), dict(cov=3001), dict(cov=300000), dict(z2=fm.Z2["0.90"]), dict(z2=fm.Z2["0.99"])])
def test_the_cap_the_cut_off_and_the_quantile(kw):
    n = 9
    thr, ref = panel()
    off, cell, w = lists()
    exp = fm.fraction_model(cohort(n), P, thr, ref, off, cell, w, kw.get("cov", COV), kw.get("vaf", 1000), kw.get("z2", fm.Z2_95))
    rc, est, count = host_fraction(cohort(n), P, thr, ref, off, cell, w, **kw)
    assert rc == 0 and same((est, count), exp)
    base = expected(n)
    if "vaf" in kw:  # the cap takes the list whose every read is the listed base, and more
        assert (count[:, LIST_FULL, fm.N_EVAL] == 0).all() and (est[:, LIST_FULL] == fm.NA).all() and (count[:, :, 0] < base[1][:, :, 0]).any()
    if "z2" in kw:
        assert not np.array_equal(est[:, :, fm.F_HI], base[0][:, :, fm.F_HI]) and np.array_equal(bits(est[:, :, fm.F_HAT]), bits(base[0][:, :, fm.F_HAT]))
    if kw.get("cov") == 300000:
        assert (est == fm.NA).all() and (count == 0).all()


def test_offsets_beyond_W_a_stride_and_deep_records():
    n = 3
    thr, ref = panel()
    off, cell, w = lists()
    W = int(off[6]) + 10  # list 6 is cut, the later ones are empty
    exp = fm.fraction_model(cohort(n), P, thr, ref, off, cell[:W], w[:W], COV, 1000)
    rc, est, count = host_fraction(cohort(n), P, thr, ref, off, cell, w, W=W)
    assert rc == 0 and same((est, count), exp) and (count[:, 7:] == 0).all() and (est[:, 7:] == fm.NA).all() and (count[:, 6, 0] > 0).any()
    wide = np.concatenate([cohort(n), cohort(n)[:, :7]], axis=1)
    rc, est, count = host_fraction(wide, P, thr, ref, off, cell, w, stride=P + 7)
    assert rc == 0 and same((est, count), expected(n))
    deep = big_records(P, n)  # int32 fields of 2^30 and 2^31 - 1
    exp = fm.fraction_model(deep, P, thr, ref, off, cell, w, COV, 1000)
    rc, est, count = host_fraction(deep, P, thr, ref, off, cell, w)
    assert rc == 0 and same((est, count), exp) and (count[:, :, 0] > 0).any() and (deep == (1 << 31) - 1).any() and (deep == 1 << 30).any()


def test_verdicts_and_changes():
    L = host_lib()
    V, Ch = L.ampli_host_fraction_verdict, L.ampli_host_fraction_change
    assert V(4, 0.1, 0.05, 5) == fm.NOT_EVALUABLE and V(5, 0.1, 0.05, 5) == fm.QUANTIFIED and V(5, 0.1, 0.0, 5) == fm.BELOW
    assert V(5, 0.0, 0.0, 5) == fm.BELOW and V(5, fm.NA, fm.NA, 0) == fm.NOT_EVALUABLE and V(0, fm.NA, fm.NA, 0) == fm.NOT_EVALUABLE
    assert V(5, 0.1, np.nextafter(0.0, 1.0), 5) == fm.QUANTIFIED
    rng = np.random.default_rng(26)
    for _ in range(3000):
        a, b = np.sort(rng.random(3) * 10.0 ** rng.integers(-5, 1)), np.sort(rng.random(3) * 10.0 ** rng.integers(-5, 1))
        a, b = np.array([a[1], a[0], a[2], 0.0]), np.array([b[1], b[0], b[2], 0.0])
        if rng.random() < 0.1:
            a[:2] = 0.0
        if rng.random() < 0.05:
            b[1] = a[2]  # equality is STABLE, not RISING
        va, vb = int(rng.integers(0, 3)), int(rng.integers(0, 3))
        ratio = C.c_double(7.0)
        code = Ch(va, _p(a), vb, _p(b), C.byref(ratio))
        want = fm.change(va, a, vb, b)
        assert code == want[0] and np.float64(ratio.value).tobytes() == np.float64(want[1]).tobytes()
    one, two = np.array([0.003, 0.002, 0.004, 9.0]), np.array([0.001, 0.0005, 0.0015, 5.0])
    ratio = C.c_double(0.0)
    assert Ch(fm.QUANTIFIED, _p(one), fm.QUANTIFIED, _p(two), C.byref(ratio)) == fm.FALLING and ratio.value == 0.001 / 0.003
    assert Ch(fm.QUANTIFIED, _p(two), fm.QUANTIFIED, _p(one), C.byref(ratio)) == fm.RISING and ratio.value == 0.003 / 0.001
    assert Ch(fm.QUANTIFIED, _p(one), fm.BELOW, _p(one), C.byref(ratio)) == fm.STABLE and ratio.value == 1.0
    assert Ch(fm.NOT_EVALUABLE, _p(one), fm.BELOW, _p(two), C.byref(ratio)) == fm.CHANGE_NOT_EVALUABLE and ratio.value == fm.NA
    zero = np.array([0.0, 0.0, 0.001, -1.0])
    assert Ch(fm.BELOW, _p(zero), fm.QUANTIFIED, _p(one), C.byref(ratio)) == fm.RISING and ratio.value == fm.NA
    assert Ch(fm.BELOW, None, fm.BELOW, _p(one), C.byref(ratio)) == -1 and Ch(fm.BELOW, _p(one), fm.BELOW, _p(one), None) == -1


def test_refusals_leave_the_outputs_untouched():
    n = 3
    thr, ref = panel()
    off, cell, w = lists()
    cases = ((dict(cov=-1), -1), (dict(vaf=-1), -1), (dict(vaf=1001), -1), (dict(stride=P - 1), -1), (dict(W=-1), -1), (dict(W=1 << 28), -6),
             (dict(z2=0.0), -1), (dict(z2=-1.0), -1), (dict(z2=np.nan), -1), (dict(z2=np.inf), -1))
    for kw, want in cases:
        rc, est, count = host_fraction(cohort(n), P, thr, ref, off, cell, w, **kw)
        assert rc == want and np.isnan(est).all() and (count == -7).all(), kw
    rc, est, count = host_fraction(cohort(n), P, thr, ref, off, cell, w, L=-1)
    assert rc == -1
    rc, est, count = host_fraction(cohort(n), P, thr, ref, off, cell, w, L=0)
    assert rc == 0
    args = [np.ascontiguousarray(x) for x in (cohort(n), thr, ref, off, cell, w)]
    prm = FractionParams(COV, 1000, fm.Z2_95)
    est, count = np.full((n, len(off) - 1, 4), np.nan), np.full((n, len(off) - 1, 2), -7, np.int64)
    full = [_p(args[0]), n, 0, P, _p(args[1]), _p(args[2]), _p(args[3]), _p(args[4]), _p(args[5]), len(off) - 1, len(cell), C.byref(prm), _p(est), _p(count)]
    for k in (0, 4, 5, 6, 7, 8, 11, 12, 13):  # every pointer
        a = list(full)
        a[k] = None
        assert host_lib().ampli_host_fraction(*a) == -1 and np.isnan(est).all() and (count == -7).all(), k
    assert host_lib().ampli_host_fraction(*full) == 0 and not np.isnan(est).any() and (count != -7).all()


def test_the_struct_and_the_constants_against_the_compiler(tmp_path):
    names = ["AMPLI_TF_F_HAT", "AMPLI_TF_F_LO", "AMPLI_TF_F_HI", "AMPLI_TF_T0", "AMPLI_TF_VALS", "AMPLI_TF_N_EVAL", "AMPLI_TF_N_SEEN", "AMPLI_TF_COUNTS", "AMPLI_TF_NA",
             "AMPLI_TF_ITERS", "AMPLI_TF_Z2_90", "AMPLI_TF_Z2_95", "AMPLI_TF_Z2_99", "AMPLI_TF_NOT_EVALUABLE", "AMPLI_TF_BELOW", "AMPLI_TF_QUANTIFIED",
             "AMPLI_TF_CHANGE_NOT_EVALUABLE", "AMPLI_TF_STABLE", "AMPLI_TF_RISING", "AMPLI_TF_FALLING", "AMPLI_ABI_VERSION"]
    lines = ['#include <cstddef>', '#include <cstdio>', '#include "amplisolve_types.h"', '#include "amplisolve_hip.h"', 'int main() {',
             '    std::printf("size %zu\\n", sizeof(ampli_fraction_params));']
    lines += [f'    std::printf("{f} %zu\\n", offsetof(ampli_fraction_params, {f}));' for f, _ in FractionParams._fields_]
    lines += [f'    std::printf("{x} %.17g\\n", (double)({x}));' for x in names]
    src, exe = tmp_path / "layout.cpp", tmp_path / "layout"
    src.write_text("\n".join(lines + ["    return 0;", "}", ""]))
    subprocess.run(["g++", *build.CXX_FLAGS, "-I", build.INCLUDE, "-o", str(exe), str(src)], check=True)
    seen = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert [f for f, _ in FractionParams._fields_] == ["coverage_cutoff", "max_vaf_pm", "z2"]
    assert int(seen["size"]) == C.sizeof(FractionParams) == 16
    for f, _ in FractionParams._fields_:
        assert int(seen[f]) == getattr(FractionParams, f).offset
    for x in names:
        assert float(seen[x]) == CONSTANTS[x], x
    assert CONSTANTS["AMPLI_ABI_VERSION"] == 5 and CONSTANTS["AMPLI_TF_ITERS"] == fm.ITERS == 60 and CONSTANTS["AMPLI_TF_NA"] == fm.NA
    assert (CONSTANTS["AMPLI_TF_Z2_90"], CONSTANTS["AMPLI_TF_Z2_95"], CONSTANTS["AMPLI_TF_Z2_99"]) == (fm.Z2["0.90"], fm.Z2["0.95"], fm.Z2["0.99"])
    assert (fm.F_HAT, fm.F_LO, fm.F_HI, fm.T0, fm.VALS) == tuple(CONSTANTS["AMPLI_TF_" + x] for x in ("F_HAT", "F_LO", "F_HI", "T0", "VALS"))
    assert (fm.NOT_EVALUABLE, fm.BELOW, fm.QUANTIFIED) == tuple(CONSTANTS["AMPLI_TF_" + x] for x in ("NOT_EVALUABLE", "BELOW", "QUANTIFIED"))
    assert (fm.CHANGE_NOT_EVALUABLE, fm.STABLE, fm.RISING, fm.FALLING) == tuple(CONSTANTS["AMPLI_TF_" + x] for x in ("CHANGE_NOT_EVALUABLE", "STABLE", "RISING", "FALLING"))
