"""AmpliSolveTumourFraction on the planted cohort (tests/fraction_cohorts.py, seed 1) written as text, against what the model
(tests/fraction_model.py, format_files) makes of the records and the error table the host library parses: the four files byte for byte,
in one chunk and with AMPLISOLVE_CHUNK_BYTES at one sample per chunk.

What the cohort must show is asserted on the model, not only on the bytes: every planted fraction (0.3 %, 0.1 % and 0 % in each of three
patients) lies inside its interval; the change from 0.3 % to 0.1 % is FALLING in all three patients; and no comparison that decides a
change (F_LO_B against F_HI_A, F_HI_B against F_LO_A) lies within 1e-9 relative -- F_LO against zero is exact, N_EVAL against
min_variants an integer comparison -- so the printed verdicts do not hang on a last bit.

Measured on the model, F_HAT [F_LO, F_HI] of the nine own pairs:
  PAT0  0.3 %: 0.00307 [0.00247, 0.00378]   0.1 %: 0.00110 [0.00069, 0.00162]   0 %: 0.00015 [0, 0.00056]
  PAT1  0.3 %: 0.00338 [0.00264, 0.00425]   0.1 %: 0.00104 [0.00055, 0.00166]   0 %: 0.00025 [0, 0.00077]
  PAT2  0.3 %: 0.00346 [0.00277, 0.00428]   0.1 %: 0.00100 [0.00053, 0.00160]   0 %: 0.00015 [0, 0.00059]
The six pairs at 0.3 % and 0.1 % are QUANTIFIED, the three at 0 % BELOW; 0.1 % -> 0 % is FALLING in PAT0 and STABLE in the other two
(their upper bounds at 0 % reach into the interval at 0.1 %); no list is QUANTIFIED in a sample it is not assigned to."""
import os
import subprocess

import numpy as np
import pytest

from amplisolve_amd.hostio import HostCohort, read_error_table
from tests import fraction_model as fm
from tests.fraction_cohorts import FRACTIONS, MARGIN, P, margins_ok, planted, write_cohort
from tests.test_fraction_host import host_fraction, same

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "amplisolve_amd", "bin")
EXE = "AmpliSolveTumourFraction"
FILES = ["Fraction_Change.txt", "Fraction_Matrix.txt", "Fraction_Own.txt", "Fraction_Summary.txt"]
COV, MIN_VARIANTS = 100, 5


def _run(args, cwd, **env):
    e = dict(os.environ, **env)
    e.pop("AMPLISOLVE_LIST_DIR_AS", None)
    return subprocess.run([os.path.join(BIN, EXE)] + args, capture_output=True, text=True, cwd=cwd, env=e)


def _args(out, d):
    return ["errorFile=table.txt", f"sample_dir={d / 'S'}", "variants=variants.txt", "assign=assign.txt", f"coverage_cutoff={COV}", f"min_variants={MIN_VARIANTS}",
            "max_vaf=1", "confidence=0.95", f"output_dir={out}"]


def test_the_four_texts_equal_the_model_in_one_and_in_many_chunks(tmp_path, monkeypatch):
    d = tmp_path
    monkeypatch.delenv("AMPLISOLVE_LIST_DIR_AS", raising=False)
    lists, assign = write_cohort(d)
    truth = planted()[4]
    # the model, from what the host library reads
    ref, thr = read_error_table(str(d / "table.txt"))
    S = HostCohort(str(d / "table.txt"), str(d / "S"), is_error_table=True)
    assert S.P == P and len(S.names) == 13 and "EMPTY" in S.names
    recs = np.ascontiguousarray(S.recs[:, :P])
    names, lnames = list(S.names), list(lists)
    off = np.concatenate([[0], np.cumsum([len(lists[n]) for n in lnames])]).astype(np.uint32)
    cell = np.array([4 * p + y for n in lnames for p, y, _ in lists[n]], np.uint32)
    w = np.array([np.float32(t) for n in lnames for _, _, t in lists[n]], np.float32)
    assert len(cell) == 43 and cell[0] == cell[14] and ((w >= 0.2) & (w <= 0.6)).all()  # one line of the first list is written twice
    est, count = fm.fraction_model(recs, P, thr, ref, off, cell, w, COV, 1000)
    rc, h_est, h_count = host_fraction(recs, P, thr, ref, off, cell, w)
    assert rc == 0 and same((h_est, h_count), (est, count))
    own = [(names.index(s), lnames.index(l)) for s, l in assign]
    params = dict(coverage_cutoff=COV, min_variants=MIN_VARIANTS, max_vaf_pm=1000, confidence="0.95")
    exp, verdicts, changes = fm.format_files(names, lnames, len(cell), P, own, est, count, params)
    print(exp["Fraction_Summary.txt"] + exp["Fraction_Own.txt"] + exp["Fraction_Change.txt"])

    # what the cohort shows, on the model
    for (s, l), (name, _) in zip(own, assign):
        assert est[s, l, fm.F_LO] <= truth[name] <= est[s, l, fm.F_HI], (name, est[s, l])
        assert verdicts[s, l] == (fm.QUANTIFIED if truth[name] > 0 else fm.BELOW), (name, est[s, l])
    assert len(changes) == 6 and [c for _, c, _ in changes[0::2]] == [fm.FALLING] * 3  # 0.3 % -> 0.1 % in every patient
    assert [c for _, c, _ in changes[1::2]] == [fm.FALLING, fm.STABLE, fm.STABLE]        # 0.1 % -> 0 %: measured
    for k, _, ratio in changes[0::2]:
        assert 0.2 < ratio < 0.5  # planted: 1 / 3
    assert margins_ok(own, est, count, MIN_VARIANTS) and MARGIN == 1e-9 and FRACTIONS == (0.003, 0.001, 0.0)
    assigned = np.zeros(verdicts.shape, bool)
    for s, l in own:
        assigned[s, l] = True
    assert ((verdicts == fm.QUANTIFIED) & ~assigned).sum() == 0  # no list is QUANTIFIED in a sample it is not assigned to: measured
    assert (verdicts[names.index("EMPTY")] == fm.NOT_EVALUABLE).all() and (est[names.index("EMPTY")] == fm.NA).all()

    r = _run(_args("one", d), d)
    assert r.returncode == 0, r.stdout[-800:] + r.stderr[-300:]
    assert "13 files in 1 chunks x 3 lists, 9 assigned pairs" in r.stdout, r.stdout[-400:]
    assert sorted(os.listdir(d / "one")) == FILES
    for name in FILES:
        assert (d / "one" / name).read_text() == exp[name], name
    r = _run(_args("chunks", d), d, AMPLISOLVE_CHUNK_BYTES="1", AMPLISOLVE_THREADS="1")
    assert r.returncode == 0 and "13 files in 13 chunks" in r.stdout, r.stdout[-800:] + r.stderr[-300:]  # one sample per chunk
    for name in FILES:  # chunks change no byte
        assert (d / "chunks" / name).read_bytes() == (d / "one" / name).read_bytes(), name
