"""AmpliSolveInSilicoDilution on the planted series (tests/dilution_cohorts.py, seed 22) written as ASEQ text, against what the model
(tests/dilution_model.py, format_files) makes of the records the host library parses and of the error table AmpliSolveErrorEstimation
writes for the 24 normals: the integer and text columns byte for byte, the float columns to 1e-5 plus a unit of the last printed digit.
Three runs -- one chunk and batch; several chunks (AMPLISOLVE_CHUNK_BYTES=7000, AMPLISOLVE_THREADS=2); one mixture a batch
(AMPLISOLVE_DILUTION_BATCH=1) -- give the same bytes, and with write_counts=1 the mixtures read back through the host's cohort reader
hold the model's integers.

Measured on the model (seed 22, 200 positions of which ten are listed twice, 24 normals, two tumours with six variants each at 5 %,
8 replicates, coverage_cutoff 100; DESIGN 22 has the table): every line has its tumour's six planted variants as truth cells and nothing
else; of the 96 (variant, replicate) pairs of the two tumour-in-normal pairs 96, 96, 94, 14 and 0 are detected at fractions 0.5, 0.2, 0.1,
0.04 and 0.02; down-sampling to a tenth keeps all; 3 novel cells in 112 mixtures, all in the down-sampled files; nothing is detected in
a mixture with a header-only file.  MEASURED below holds the figures per line; the device is held to those integers exactly."""
import os
import subprocess

import numpy as np
import pytest

from amplisolve_amd.hostio import HostCohort, read_error_table
from tests import dilution_model as dm
from tests.dilution_cohorts import FRACTIONS_CLI, SERIES_SEED, series_lines, write_series
from tests.test_dilution_host import host_dilute

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "amplisolve_amd", "bin")
FILES = ["Dilution_Lines.txt", "Dilution_Summary.txt", "Dilution_Variants.txt"]
REPLICATES, COV, CONF = 8, 100, 0.95
FLOAT_COLS = {"Dilution_Variants.txt": (11, 12, 15, 16), "Dilution_Lines.txt": (5, 6, 7, 9, 10)}
# per line of series_lines(): (truth cells, detections over the 8 replicates, novel cells over the 8 replicates), measured on the model
MEASURED = [(6, 48, 0), (6, 48, 0), (6, 48, 0), (6, 11, 0), (6, 0, 0), (6, 48, 2), (6, 48, 0), (6, 48, 0), (6, 46, 0), (6, 3, 0), (6, 0, 0), (6, 48, 1),
            (6, 48, 0), (6, 0, 0)]


def _run(exe, args, cwd, **env):
    e = dict(os.environ, **env)
    e.pop("AMPLISOLVE_LIST_DIR_AS", None)
    return subprocess.run([os.path.join(BIN, exe)] + args, capture_output=True, text=True, cwd=cwd, env=e)


def _args(table, out, write_counts=0):
    return [f"errorFile={table}", "sample_dir=S", "mixtures=mixtures.txt", f"replicates={REPLICATES}", f"seed={SERIES_SEED}", f"coverage_cutoff={COV}",
            f"confidence={CONF}", f"write_counts={write_counts}", f"output_dir={out}"]


def _host_mix(recs_a, recs_b, P, mixtures):
    rc, out, flags = host_dilute(np.ascontiguousarray(recs_a), np.ascontiguousarray(recs_b), P, mixtures)
    assert rc == 0
    return out, flags


def _same(got, want, name):
    g, w = [l.split("\t") for l in got.split("\n")], [l.split("\t") for l in want.split("\n")]
    assert len(g) == len(w) and g[0] == w[0] and g[-1] == w[-1] == [""], name
    for a, b in zip(g[1:-1], w[1:-1]):
        assert len(a) == len(b), (a, b)
        for c, (x, y) in enumerate(zip(a, b)):
            if c in FLOAT_COLS.get(name, ()) and x != y:
                digits = len(y.split(".")[1])
                assert abs(float(x) - float(y)) <= 1e-5 + 10.0 ** -digits, (name, c, a, b)
            else:
                assert x == y, (name, c, a, b)


def test_the_three_texts_equal_the_model_in_one_and_in_many_batches(tmp_path, monkeypatch):
    d = tmp_path
    monkeypatch.delenv("AMPLISOLVE_LIST_DIR_AS", raising=False)
    monkeypatch.delenv("AMPLISOLVE_DILUTION_BATCH", raising=False)
    variants = write_series(d)
    r = _run("AmpliSolveErrorEstimation", ["panel_design=p.bed", "reference_genome=x.fa", "germline_dir=N", "C_value=0.002", f"coverage_cutoff={COV}",
                                           "default_error=0.01", "output_dir=o"], d, AMPLISOLVE_REFBASES_FILE="r.txt")
    assert r.returncode == 0, r.stdout[-600:] + r.stderr[-300:]
    table = "o/" + [n for n in os.listdir(d / "o") if n.startswith("positionSpecificNoise_")][0]
    # the model, from what the host library reads
    ref, thr = read_error_table(str(d / table))
    S = HostCohort(str(d / table), str(d / "S"), is_error_table=True)
    P = S.P
    assert P == 200 and sorted(S.names) == ["DIL0", "DIL1", "EMPTY", "TUM0", "TUM1"] and (ref > 3).sum() >= 3
    recs = np.ascontiguousarray(S.recs[:, :P])
    positions = [S.position(p) for p in range(P)]
    lines = series_lines()
    exp, res = dm.format_files(S.names, positions, ref, recs, thr, lines, REPLICATES, SERIES_SEED, COV, CONF, mix=_host_mix)
    figures = [(len(x["truth"]), sum(x["detected"]), sum(x["novel"])) for x in res]
    print("per line (truth cells, detections, novel cells):", figures)
    print(exp["Dilution_Summary.txt"] + exp["Dilution_Lines.txt"])
    rate = {f: sum(sum(x["detected"]) for x in res if x["line"][2] == f and x["line"][1].startswith("DIL") and x["line"][3] == 1.0) for f in FRACTIONS_CLI}
    print("detections per fraction over both pairs:", rate)
    planted = {(f"TUM{t}", p, y) for t, p, y in variants}
    for x in res:  # the truth cells of a tumour are its planted variants and nothing else
        assert {(x["line"][0], p, nt) for p, nt in x["truth"]} == {v for v in planted if v[0] == x["line"][0]}, x["line"]

    r = _run("AmpliSolveInSilicoDilution", _args(table, "one", write_counts=1), d)
    assert r.returncode == 0, r.stdout[-800:] + r.stderr[-300:]
    assert "of 5 files in 1 chunks, 14 batches" in r.stdout, r.stdout[-400:]
    assert sorted(os.listdir(d / "one")) == FILES + ["mixtures"]
    for name in FILES:
        _same((d / "one" / name).read_text(), exp[name], name)
    r = _run("AmpliSolveInSilicoDilution", _args(table, "chunks"), d, AMPLISOLVE_CHUNK_BYTES="7000", AMPLISOLVE_THREADS="2")
    assert r.returncode == 0 and "of 5 files in 1 chunks" not in r.stdout and "14 batches" in r.stdout, r.stdout[-800:] + r.stderr[-300:]
    r = _run("AmpliSolveInSilicoDilution", _args(table, "single"), d, AMPLISOLVE_DILUTION_BATCH="1")
    assert r.returncode == 0 and f"{14 * REPLICATES} batches" in r.stdout, r.stdout[-800:] + r.stderr[-300:]
    for name in FILES:  # chunks and batches change nothing: a mixture's bytes do not depend on the batch it is made in
        assert (d / "chunks" / name).read_bytes() == (d / "one" / name).read_bytes() == (d / "single" / name).read_bytes(), name

    # write_counts=1: every mixture as a count file that any other command can read
    M = HostCohort(str(d / table), str(d / "one" / "mixtures"), is_error_table=True)
    assert M.S == len(lines) * REPLICATES
    row = {n: i for i, n in enumerate(M.names)}
    for li, x in enumerate(res):
        for rep in range(REPLICATES):
            got = M.recs[row[f"L{li + 1:03d}_R{rep:04d}"], :P]
            assert np.array_equal(got, x["out"][rep]), (li, rep)
    # what the cohort shows, as measured on the model
    assert list(rate.values()) == sorted(rate.values(), reverse=True)  # the rate falls with the fraction, in aggregate
    assert figures == MEASURED
