"""AmpliSolveDetectionPower on a fresh panel (two overlapping amplicons, so positions listed twice; 3 tumour files): its MinReads and Status
columns are AmpliSolveDetectionLimit's, its Power and LoD columns the definition's (tests/power_model.py) within the tolerances of
DESIGN 12, its summary consistent with its rows, and what it refuses."""
import os
import subprocess

import numpy as np
import pytest

from tests import power_model as pm
from tests.helpers import write_fresh_panel, write_fresh_tumours

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "amplisolve_amd", "bin")
LEVELS = ("0.002", "0.005", "0.02")
CONF = "0.95"
TAIL_TOL, LOD_TOL, BAND = 1e-6, 1e-4, 2e-6


def _run(exe, args, cwd, **env):
    return subprocess.run([os.path.join(BIN, exe)] + args, capture_output=True, text=True, cwd=cwd, env=dict(os.environ, **env))


def test_power_files_equal_the_limits_files_and_the_model(tmp_path):
    d = tmp_path
    write_fresh_panel(d, 91, depth=2000, S=6, amplicons=2)
    write_fresh_tumours(d, 91, T=3, depth=2000)
    r = _run("AmpliSolveErrorEstimation", ["panel_design=p.bed", "reference_genome=x.fa", "germline_dir=N", "C_value=0.002", "coverage_cutoff=100",
                                           "default_error=0.01", "output_dir=o"], d, AMPLISOLVE_REFBASES_FILE="r.txt")
    assert r.returncode == 0, r.stdout[-600:] + r.stderr[-300:]
    table = "o/" + [n for n in os.listdir(d / "o") if n.startswith("positionSpecificNoise_")][0]
    common = [f"errorFile={table}", "tumour_dir=T", "coverage_cutoff=100", "levels=" + ",".join(LEVELS)]
    r = _run("AmpliSolveDetectionLimit", common[:2] + ["output_dir=dl"] + common[2:], d)
    assert r.returncode == 0, r.stdout[-800:]
    r = _run("AmpliSolveDetectionPower", common[:2] + ["output_dir=dp"] + common[2:] + [f"confidence={CONF}"], d)
    assert r.returncode == 0, r.stdout[-800:]
    c32 = float(np.float32(float(CONF)))
    levels = tuple(float(v) for v in LEVELS)
    rng = np.random.default_rng(3)
    summary = [l.split("\t") for l in (d / "dp" / "Summary_Detection_Power.txt").read_text().splitlines()]
    assert summary[0] == ["Filename", "Lines", "Pairs", "OK", "MedianLoD"] + [f"Power@{v}>={CONF}" for v in LEVELS]
    by_name = {g[0]: g[1:] for g in summary[1:]}
    names = sorted(f[: -len("_detection_power.txt")] for f in os.listdir(d / "dp") if f.endswith("_detection_power.txt"))
    assert len(names) == 3 and set(names) == set(by_name)
    worst_p = worst_l = 0.0
    statuses = set()
    for name in names:
        rows = [l.split("\t") for l in (d / "dp" / f"{name}_detection_power.txt").read_text().splitlines()]
        lim = [l.split("\t") for l in (d / "dl" / f"{name}_detection_limits.txt").read_text().splitlines()]
        assert rows[0] == ["Chrom", "Position", "Ref", "Alt", "RD_fw", "RD_bw", "MinReads_fw", "MinReads_bw", "Status", "LoD"] + [f"Power@{v}" for v in LEVELS]
        rows, lim = rows[1:], lim[1:]
        assert len(rows) == len(lim) > 600
        ok_rows = []
        for g, h in zip(rows, lim):  # limits: Chrom Position Ref Alt RD RD_fw RD_bw Thr_fw Thr_bw MinReads_fw MinReads_bw MinAF Status ...
            assert g[:4] == h[:4] and g[4:6] == h[5:7] and g[6:8] == h[9:11] and g[8] == h[12], (g, h)
            if g[8] == "OK":
                ok_rows.append(g)
            else:
                assert g[6:8] == [".", "."] and g[9:] == ["."] * (1 + len(LEVELS)), g
        assert len(ok_rows) > 300
        statuses |= {g[8] for g in rows}
        lo, hi = np.zeros(len(LEVELS), np.int64), np.zeros(len(LEVELS), np.int64)
        for g in ok_rows:
            cell = (int(g[4]), int(g[6]), int(g[5]), int(g[7]))
            want = pm.powers(*cell, levels)
            worst_p = max(worst_p, max(abs(float(a) - b) for a, b in zip(g[10:], want)))
            lo += np.array(want) >= c32 + BAND
            hi += np.array(want) >= c32 - BAND
        for i in rng.permutation(len(ok_rows))[:150]:  # a pure-Python root search is ~100 tails
            g = ok_rows[i]
            worst_l = max(worst_l, abs(float(g[9]) / pm.lod(int(g[4]), int(g[6]), int(g[5]), int(g[7]), c32) - 1))
        s = by_name[name]
        n_lines = sum(1 for _ in open(d / "T" / next(f for f in os.listdir(d / "T") if f.startswith(name + ".")))) - 1
        assert [int(s[0]), int(s[1]), int(s[2])] == [n_lines, len(rows), len(ok_rows)]
        lods = sorted(float(g[9]) for g in ok_rows)
        assert abs(float(s[3]) / lods[(len(lods) - 1) // 2] - 1) <= 1e-5  # the lower median, printed with six digits
        counts = np.array([int(v) for v in s[4:]])
        assert (hi - lo).sum() <= 0.01 * len(ok_rows)
        assert (lo <= counts).all() and (counts <= hi).all() and (np.diff(counts) >= 0).all() and counts[-1] > 0, (lo, counts, hi)
    assert statuses >= {"OK", "LOWDEPTH"}
    print(f"against the model: power {worst_p:.3g}, LoD {worst_l:.3g} relative")
    assert worst_p <= TAIL_TOL and worst_l <= LOD_TOL


def test_command_line_refusals(tmp_path):
    r = _run("AmpliSolveDetectionPower", ["errorFile=x", "tumour_dir=y"], tmp_path)
    assert r.returncode == 1 and "Usage" in r.stdout
    for levels, conf, env in (("0.01", "0.4", {}), ("0.01", "0.995", {}), ("0.01", "", {}), ("0.01", "0.9x", {}), ("0.01,2", "0.95", {}), ("", "0.95", {}),
                              (",".join(["0.01"] * 9), "0.95", {}), ("0.01", "0.95", {"AMPLISOLVE_WORLD_SIZE": "2"})):
        r = _run("AmpliSolveDetectionPower", ["errorFile=x", "tumour_dir=y", f"output_dir={tmp_path}/o", "coverage_cutoff=100", f"levels={levels}",
                                              f"confidence={conf}"], tmp_path, **env)
        assert r.returncode == 1 and "failed" in r.stdout, (levels, conf)
        assert not os.path.exists(tmp_path / "o")  # refused before anything is written
