"""AmpliSolveFalseDiscovery on the planted cohort (tests/fdr_cohorts.py) written as ASEQ text, against what the model (tests/fdr_model.py,
format_files) makes of the plane the project's own scorer gives for the records the host library parses: the text columns, the counts,
the ranks and the raw-gate column byte for byte, the float columns to 1e-5 plus a unit of the last printed digit.  The scorer itself is
held to its model in tests/test_gpu_overdispersion.py; here its plane is the input, so that ranks and ties are the same integers.  One
run in a single chunk and batch, one in three chunks (AMPLISOLVE_CHUNK_BYTES) and one-row batches (AMPLISOLVE_FDR_BATCH_ROWS): the same
bytes.

Measured on the model (seed 21, 300 positions, 24 normals, 5 tumours, background 0.1 %, 25 variants at 0.3 % to 5 %, fdr 0.05, q_min
13; DESIGN 21 has the table): 19 of the 25 planted variants are listed (all 15 at 1 % and above, 4 of 5 at 0.5 %, none of 5 at 0.3 %; the
raw gate passes 21: one more at each of 0.5 % and 0.3 %), and of the 4475 background cells none passes the raw gate or the adjusted one
-- the background lies at a third of the table's threshold (rate + C_value).  m = 900 tested cells in every file."""
import os
import subprocess

import numpy as np
import pytest

from amplisolve_amd.hostio import HostCohort
from tests import fdr_model as fm
from tests.fdr_cohorts import planted
from tests.test_gpu_loo import _pack
from tests.test_gpu_overdispersion import _chunks
from tests.test_gpu_parity import _t

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "amplisolve_amd", "bin", "AmpliSolveFalseDiscovery")
HEADER = "chr\tpos\tdbsnp\tMAF\tref\talt\tA\tC\tG\tT\tRD\tArs\tCrs\tGrs\tTrs\n"
FILES = ["FDR_Calls.txt", "FDR_Samples.txt", "FDR_Summary.txt"]
PARAMS = dict(C_value=0.002, coverage_cutoff=100, calling_cutoff=100, fdr=0.05, q_min=13.0)
KEYS = ["C_value", "coverage_cutoff", "calling_cutoff", "fdr", "q_min"]
START = 1000
PLANTED_FOUND, BACKGROUND_RAW, BACKGROUND_ADJ = 19, 0, 0  # measured on the model, see the docstring
TEXT = (0, 1, 2, 3, 4, 5, 6, 7, 13, 14)
# Q, Key and A are printed with six decimals: 1e-5 and a unit of the sixth; q = 10^(-A / 10) with six digits: relative, d ln q = 0.23 dA
ABS_TOL, REL_TOL = {8: 1.1e-5, 9: 1.1e-5, 10: 1.1e-5, 11: 1.1e-5}, {12: 1e-5}


def _write(d):
    normals, tumours, ref, variants = planted()
    P = normals.shape[1]
    (d / "p.bed").write_text(f"chr7\t{START}\t{START + P - 1}\n")
    (d / "r.txt").write_text("".join(f"chr7\t{START + p}\t{'ACGT'[ref[p]]}\n" for p in range(P)))
    for sub, recs, stem in (("N", normals, "NORM"), ("T", tumours, "TUM")):
        (d / sub).mkdir()
        for s in range(recs.shape[0]):
            text = HEADER
            for p in range(P):
                r = recs[s, p].astype(np.int64)
                tot = r[:4] + r[4:]
                text += f"chr7\t{START + p}\t.\t.\t.\t.\t{tot[0]}\t{tot[1]}\t{tot[2]}\t{tot[3]}\t{tot.sum()}\t{r[4]}\t{r[5]}\t{r[6]}\t{r[7]}\n"
            (d / sub / f"{stem}{s:02d}.PILEUP.ASEQ").write_text(text)
    return variants


def _run(args, cwd, **env):
    e = dict(os.environ, **env)
    e.pop("AMPLISOLVE_LIST_DIR_AS", None)
    return subprocess.run([EXE] + args, capture_output=True, text=True, cwd=cwd, env=e)


def _args(d, out, **kw):
    p = dict(PARAMS, **kw)
    return [f"panel_design={d / 'p.bed'}", "reference_genome=unused.fa", f"germline_dir={d / 'N'}", f"tumour_dir={d / 'T'}"] + [f"{k}={p[k]}" for k in KEYS] + [
        f"output_dir={d / out}"]


def _model(ctx, d, variants):
    normals = HostCohort(str(d / "p.bed"), str(d / "N"), refbases_file=str(d / "r.txt"))
    tumours = HostCohort(str(d / "p.bed"), str(d / "T"), refbases_file=str(d / "r.txt"))
    P = normals.P
    assert normals.E == 0 and tumours.S == 5 and normals.S == 24
    ref = normals.ref_code.copy()
    rec = _chunks(ctx, normals.recs, P, 0, None, None, None, "i32", (0, normals.S))[0]
    table = ctx.error_reduce_records(rec, P, ctx.new_acc(P), PARAMS["C_value"], PARAMS["coverage_cutoff"], finalize=True)
    rt = ctx.records(_pack(ctx, tumours.recs, "i32"), "i32", tumours.S)
    q = ctx.nb_score(rt, P, table.thr, _t(ref), None, PARAMS["calling_cutoff"]).cpu().numpy()
    A, m, R = fm.adjust(q, False)
    a_min = -10.0 * np.log10(PARAMS["fdr"])
    assert not ((A != fm.NA) & (np.abs(A - a_min) <= 2e-5)).any()  # no A of this cohort sits where the listing could turn
    # what the listing finds: by the tumours' names, since the files are visited in an order of their own
    row = {name: i for i, name in enumerate(tumours.names)}
    found = (A != fm.NA) & (A.astype(np.float32) >= a_min)
    raw = (A != fm.NA) & (q[..., 0] >= PARAMS["q_min"]) & (q[..., 1] >= PARAMS["q_min"])
    is_var = np.zeros(found.shape, bool)
    for t, p, b, vaf in variants:
        is_var[row[f"TUM{t:02d}"], p, b] = True
    by_vaf = {}
    for t, p, b, vaf in variants:
        hit = by_vaf.setdefault(vaf, [0, 0, 0])
        hit[0] += 1
        hit[1] += bool(found[row[f"TUM{t:02d}"], p, b])
        hit[2] += bool(raw[row[f"TUM{t:02d}"], p, b])
    figures = (int((found & is_var).sum()), int((raw & ~is_var).sum()), int((raw & found & ~is_var).sum()))
    print("planted found / background raw / background raw and adjusted:", figures, "background adjusted:", int((found & ~is_var).sum()),
          "m", m.tolist(), "by fraction (planted, adjusted, raw):", by_vaf)
    positions = [("chr7", START + p) for p in range(P)]
    return fm.format_files(tumours.names, normals.S, positions, ref, tumours.recs, q, PARAMS), figures


def _same(d, out, exp):
    assert sorted(os.listdir(d / out)) == FILES
    for name in ("FDR_Samples.txt", "FDR_Summary.txt"):
        got, want = (d / out / name).read_text(), exp[name]
        if name == "FDR_Samples.txt":  # MinKey is a float column
            g, w = [l.split("\t") for l in got.split("\n")], [l.split("\t") for l in want.split("\n")]
            assert [x[:5] for x in g] == [x[:5] for x in w]
            assert all(a[5] == b[5] or abs(float(a[5]) - float(b[5])) <= 1.1e-5 for a, b in zip(g[1:-1], w[1:-1]))
        else:
            assert got == want, name
    got, want = (d / out / "FDR_Calls.txt").read_text().split("\n"), exp["FDR_Calls.txt"].split("\n")
    assert len(got) == len(want) and got[0] == want[0] and got[-1] == want[-1] == ""
    for g, w in zip(got[1:-1], want[1:-1]):
        g, w = g.split("\t"), w.split("\t")
        assert len(g) == len(w) == 15 and all(g[c] == w[c] for c in TEXT), (g, w)
        for c, tol in ABS_TOL.items():
            assert abs(float(g[c]) - float(w[c])) <= tol, (c, g, w)
        for c, tol in REL_TOL.items():
            assert abs(float(g[c]) - float(w[c])) <= tol * float(w[c]), (c, g, w)


def test_files_equal_the_model_in_one_and_in_many_batches(ctx, tmp_path, monkeypatch):
    d = tmp_path
    monkeypatch.delenv("AMPLISOLVE_LIST_DIR_AS", raising=False)
    monkeypatch.delenv("AMPLISOLVE_FDR_BATCH_ROWS", raising=False)
    variants = _write(d)
    env = dict(AMPLISOLVE_REFBASES_FILE=str(d / "r.txt"))
    exp, figures = _model(ctx, d, variants)
    print(exp["FDR_Summary.txt"] + exp["FDR_Samples.txt"])
    assert figures == (PLANTED_FOUND, BACKGROUND_RAW, BACKGROUND_ADJ)
    r = _run(_args(d, "one"), d, **env)
    assert r.returncode == 0, r.stdout[-800:] + r.stderr[-300:]
    assert "5 tumours in 1 chunks against 24 normals" in r.stdout and "adjusted in 1 batches of at most 5 rows (AMPLISOLVE_FDR_BATCH_ROWS)" in r.stdout, r.stdout[-400:]
    _same(d, "one", exp)
    r = _run(_args(d, "many"), d, AMPLISOLVE_CHUNK_BYTES="7000", AMPLISOLVE_THREADS="2", AMPLISOLVE_FDR_BATCH_ROWS="1", **env)
    assert r.returncode == 0, r.stdout[-800:] + r.stderr[-300:]
    assert "5 tumours in 3 chunks against 24 normals" in r.stdout and "adjusted in 5 batches of at most 1 rows (AMPLISOLVE_FDR_BATCH_ROWS)" in r.stdout, r.stdout[-400:]
    for name in FILES:  # chunks and batches change nothing: a row's bytes do not depend on the rows beside it
        assert (d / "many" / name).read_bytes() == (d / "one" / name).read_bytes(), name


def test_exit_status_and_refusals_on_the_device(tmp_path):
    d = tmp_path
    _write(d)
    env = dict(AMPLISOLVE_REFBASES_FILE=str(d / "r.txt"))
    a = [f"germline_dir={d / 'no_such_dir'}" if x.startswith("germline_dir=") else x for x in _args(d, "o")]
    r = _run(a, d, **env)
    assert r.returncode == 1 and "failed" in r.stdout and not os.path.exists(d / "o")
    r = _run(_args(d, "o"), d, AMPLISOLVE_REFBASES_FILE=str(d / "none.txt"))
    assert r.returncode == 1 and "failed" in r.stdout and not os.path.exists(d / "o")
    r = _run(_args(d, "o", fdr=0.5, q_min=5, calling_cutoff=0, coverage_cutoff=1), d, **env)
    assert r.returncode == 0 and sorted(os.listdir(d / "o")) == FILES
