"""AmpliSolveVariantMonitoring on the planted cohort (tests/monitor_cohorts.py, seed 24) written as text, against what the model
(tests/monitor_model.py, format_files) makes of the records and the error table the host library parses: the three files byte for
byte.  The scores and the walk of the limit of detection in the expected text are the host library's (bit for bit the device's); the
50-digit model says that they decide nothing differently: no pooled Q lies within 2e-5 of q_min and no control's statistic within 2e-5
of its observed one (asserted), so verdicts and n_ge are exact.  Three runs -- one chunk and batch; several chunks
(AMPLISOLVE_CHUNK_BYTES=7000, AMPLISOLVE_THREADS=2); one control replicate a batch (AMPLISOLVE_MONITOR_BATCH=1) -- give the same bytes.

Measured on the model: 300 positions, ten files, three lists of 15, 14 and 14 entries, q_min 30, 50 controls.  The three
plasma files at 0.3 % are DETECTED (Q 73.3 / 70.3, 70.7 / 73.1, 96.9 / 94.8) while none of their 43 listed cells passes the per-cell
gate (both strands' Poisson Q >= 30); the three at 0.15 % are NOT_DETECTED (one strand reaches 34.0 and 43.5 in two of them, the other
does not: both must pass); no list detects a sample it is not assigned to (0 cross-patient false positives in 24 cells); n_ge is 0 for
every own pair; the header-only file is NOT_EVALUABLE."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from amplisolve_amd import host_lib
from amplisolve_amd.hostio import HostCohort, read_error_table
from tests import monitor_model as mm
from tests.monitor_cohorts import SEED, P, write_cohort
from tests.test_monitor_host import _p, bits, host_controls, host_score, host_sums

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "amplisolve_amd", "bin")
EXE = "AmpliSolveVariantMonitoring"
FILES = ["Monitoring_Matrix.txt", "Monitoring_Own.txt", "Monitoring_Summary.txt"]
COV, Q_MIN, MIN_VARIANTS, MIN_SEEN, R = 100, 30.0, 5, 2, 50
# per own pair in the order of assign.txt: (verdict, n_ge, listed cells that pass the per-cell gate), measured on the model
MEASURED = [(mm.DETECTED, 0, 0), (mm.NOT_DETECTED, 0, 0)] * 3


def _run(args, cwd, **env):
    e = dict(os.environ, **env)
    e.pop("AMPLISOLVE_LIST_DIR_AS", None)
    return subprocess.run([os.path.join(BIN, EXE)] + args, capture_output=True, text=True, cwd=cwd, env=e)


def _args(out, d):
    # the visit order of the files is a function of the directory as it is written: the same text as the model's reader gets
    return ["errorFile=table.txt", f"sample_dir={d / 'S'}", "variants=variants.txt", "assign=assign.txt", f"coverage_cutoff={COV}", f"q_min={Q_MIN:g}",
            f"min_variants={MIN_VARIANTS}", f"min_seen={MIN_SEEN}", "max_vaf=1", f"controls={R}", f"seed={SEED}", f"output_dir={out}"]


def test_the_three_texts_equal_the_model_in_one_and_in_many_chunks_and_batches(tmp_path, monkeypatch):
    d = tmp_path
    monkeypatch.delenv("AMPLISOLVE_LIST_DIR_AS", raising=False)
    monkeypatch.delenv("AMPLISOLVE_MONITOR_BATCH", raising=False)
    lists, assign = write_cohort(d)
    # the model, from what the host library reads
    ref, thr = read_error_table(str(d / "table.txt"))
    S = HostCohort(str(d / "table.txt"), str(d / "S"), is_error_table=True)
    assert S.P == P and len(S.names) == 10 and "EMPTY" in S.names
    recs = np.ascontiguousarray(S.recs[:, :P])
    names, lnames = list(S.names), list(lists)
    off = np.concatenate([[0], np.cumsum([len(lists[n]) for n in lnames])]).astype(np.uint32)
    cell = np.array([4 * p + y for n in lnames for p, y in lists[n]], np.uint32)
    assert len(cell) == 43 and cell[0] == cell[14]  # one line of the first list is written twice
    sums, lam = mm.sums_model(recs, P, thr, ref, off, cell, COV, 1000)
    rc, hs, hl = host_sums(recs, P, thr, ref, off, cell)
    assert rc == 0 and np.array_equal(hs, sums) and np.array_equal(bits(hl), bits(lam))
    q = host_score(sums, lam).reshape(len(names), len(lnames), 2)
    q64 = mm.score_model(sums, lam)[1]
    assert np.abs(q.astype(np.float64) - q64).max() <= 1e-5 and np.abs(q64 - Q_MIN).min() > 2e-5  # no pooled Q near q_min
    own = [(names.index(s), lnames.index(l)) for s, l in assign]
    cand_off, cand_pos = mm.candidates(ref)
    pairs = np.array(own, np.int32)
    cs, cl = mm.controls_model(recs, P, thr, ref, off, cell, pairs, cand_off, cand_pos, R, 0, SEED, COV, 1000)
    rc, hcs, hcl = host_controls(recs, P, thr, ref, off, cell, pairs, cand_off, cand_pos, R, 0, SEED)
    assert rc == 0 and np.array_equal(hcs, cs) and np.array_equal(bits(hcl), bits(cl))
    cq = host_score(cs, cl).reshape(len(own), R, 2)
    cq64 = mm.score_model(cs, cl)[1]
    L = host_lib()
    n_ge, lods, figures = [], [], []
    for k, (s, l) in enumerate(own):
        assert np.abs(cq64[k].min(axis=1) - q64[s, l].min()).min() > 2e-5  # no control's statistic near the observed one
        n_ge.append(mm.count_ge(q[s, l, 0], q[s, l, 1], cq[k]))
        assert n_ge[-1] == int((cq64[k].min(axis=1) >= q64[s, l].min()).sum())
        lods.append(L.ampli_host_monitor_lod(lam[s, l, 0], lam[s, l, 1], int(sums[s, l, mm.D_FW]), int(sums[s, l, mm.D_BW]), Q_MIN))
        if k < 2:  # the model's own walk, where it is cheap
            assert lods[-1] == mm.lod(lam[s, l, 0], lam[s, l, 1], sums[s, l, mm.D_FW], sums[s, l, mm.D_BW], Q_MIN)
        passing = 0  # the per-cell gate: both strands' Poisson Q of the cell reach q_min
        for p, y in lists[lnames[l]]:
            r = recs[s, p]
            kk, dd = np.array([r[y], r[4 + y]], np.int32), np.array([r[:4].sum(), r[4:].sum()], np.int32)
            ee, qq = np.array([thr[0, y, p], thr[1, y, p]], np.float32), np.zeros(2, np.float32)
            assert L.ampli_host_nb_score_batch(_p(kk), _p(dd), _p(ee), None, 2, _p(qq)) == 0
            passing += bool((qq >= Q_MIN).all())
        figures.append((mm.verdict(sums[s, l, 0], sums[s, l, 1], q[s, l, 0], q[s, l, 1], MIN_VARIANTS, MIN_SEEN, Q_MIN), n_ge[-1], passing))
    params = dict(coverage_cutoff=COV, q_min=Q_MIN, min_variants=MIN_VARIANTS, min_seen=MIN_SEEN, max_vaf_pm=1000, controls=R, seed=SEED)
    exp, verdicts = mm.format_files(names, lnames, len(cell), P, own, sums, lam, q, n_ge, lods, params)
    print("per own pair (verdict, n_ge, cells passing the per-cell gate):", figures)
    print(exp["Monitoring_Summary.txt"] + exp["Monitoring_Own.txt"])
    assigned = np.zeros(verdicts.shape, bool)
    for s, l in own:
        assigned[s, l] = True
    cross = int(((verdicts == mm.DETECTED) & ~assigned).sum())

    r = _run(_args("one", d), d)
    assert r.returncode == 0, r.stdout[-800:] + r.stderr[-300:]
    assert "10 files in 1 chunks x 3 lists, 6 assigned pairs x 50 controls in 1 batches" in r.stdout, r.stdout[-400:]
    assert sorted(os.listdir(d / "one")) == FILES
    for name in FILES:
        assert (d / "one" / name).read_text() == exp[name], name
    r = _run(_args("chunks", d), d, AMPLISOLVE_CHUNK_BYTES="7000", AMPLISOLVE_THREADS="2")
    assert r.returncode == 0 and "10 files in 1 chunks" not in r.stdout, r.stdout[-800:] + r.stderr[-300:]
    r = _run(_args("single", d), d, AMPLISOLVE_MONITOR_BATCH="1")
    assert r.returncode == 0 and f"in {R} batches" in r.stdout, r.stdout[-800:] + r.stderr[-300:]
    for name in FILES:  # chunks and batches change nothing
        assert (d / "chunks" / name).read_bytes() == (d / "one" / name).read_bytes() == (d / "single" / name).read_bytes(), name
    # what the cohort shows, as measured on the model
    assert figures == MEASURED and cross == 0
    assert (verdicts[names.index("EMPTY")] == mm.NOT_EVALUABLE).all()
