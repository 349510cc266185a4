"""The index arithmetic of the lgamma table (csrc/ampli_math.h: ampli_lgamma_int, ampli_lgamma_int_next) under the address and
undefined-behaviour sanitizers, on the host: tests/csrc/scorer_domain_main.cpp is compiled into a program of its own and run.  It
holds a heap table of exactly AMPLI_LGTAB entries and compares the table-backed forms of ampli_drain_p and ampli_poisson_score_dense
with their no-table forms, bit for bit, at every table index, beyond the table's end, and at the edges of the int32 domain
(k = INT32_MAX: k + 1 formed as an int wrapped to INT32_MIN, passed the signed guard and indexed 16 GB below the table).
Nothing is loaded into this process and no environment is set: the program is linked against the sanitizers' runtimes itself.

And the explicit edge points of tests/scorer_grids.py through the host's probes: both forms, and the oracle's literal scorer."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from amplisolve_amd import host_lib
from oracle import pyoracle as orc
from tests import scorer_grids

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def test_table_index_arithmetic_is_clean_under_the_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    r = subprocess.run([gxx, *FLAGS, str(probe), "-o", str(tmp_path / "probe")], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("g++ cannot link the sanitizers' runtimes: " + r.stderr.strip().splitlines()[-1][:200])
    exe = tmp_path / "scorer_domain"
    r = subprocess.run([gxx, *FLAGS, os.path.join(ROOT, "tests", "csrc", "scorer_domain_main.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-6000:])
    assert " 0 differences" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, (r.stdout, r.stderr[-6000:])


def _host(fn, k, rd, e, with_p):
    q = np.empty(k.size, np.float64)
    p = np.empty(k.size, np.float64)
    args = [k.ctypes.data_as(C.c_void_p), rd.ctypes.data_as(C.c_void_p), e.ctypes.data_as(C.c_void_p), k.size, q.ctypes.data_as(C.c_void_p)]
    fn(*args, p.ctypes.data_as(C.c_void_p)) if with_p else fn(*args)
    return q, (p if with_p else None)


def test_edge_points_on_the_host_both_forms_and_the_oracle():
    H = host_lib()
    k1, rd1, e1, above = scorer_grids.table_end_points()
    q1, _ = orc.score_batch(k1, rd1, e1)
    assert above.any() and (~above).any()
    assert ((q1[above] > 5) & (q1[above] < 100)).all(), q1[above]  # mid-range Q across the table's end
    k2, rd2, e2 = scorer_grids.edge_points()
    k, rd, e = np.concatenate([k1, k2]), np.concatenate([rd1, rd2]), np.concatenate([e1, e2])
    qo, po = orc.score_batch(k, rd, e)
    assert np.isnan(qo).any() and (qo == -888).any() and (qo == 0).any() and (qo == 100).any()
    q, _ = _host(H.ampli_host_dense_score_batch, k, rd, e, False)
    qt, _ = _host(H.ampli_host_dense_score_table_batch, k, rd, e, False)
    assert np.array_equal(q.view(np.int64), qt.view(np.int64))
    scorer_grids.compare_with_oracle("host dense", k, rd, e, qo, po, q)
    d = scorer_grids.in_drain_domain(k, rd, e)
    assert d.sum() >= 40 and (k[d] == scorer_grids.INT32_MAX).any() and (rd[d] == scorer_grids.INT32_MAX).any()
    ee = np.where(e[d] == 0, np.float32(0.0010008), e[d]).astype(np.float32)  # the drain is handed the effective error
    kd, rdd = np.ascontiguousarray(k[d]), np.ascontiguousarray(rd[d])
    qd, pd = _host(H.ampli_host_drain_score_batch, kd, rdd, ee, True)
    qdt, pdt = _host(H.ampli_host_drain_score_table_batch, kd, rdd, ee, True)
    assert np.array_equal(pd.view(np.int64), pdt.view(np.int64)) and np.array_equal(qd.view(np.int64), qdt.view(np.int64))
    scorer_grids.compare_with_oracle("host drain", kd, rdd, ee, qo[d], po[d], qd, pd)
