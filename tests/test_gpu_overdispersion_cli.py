"""AmpliSolveOverdispersedCalling on the planted cohort (tests/overdispersion_cohorts.py) written as ASEQ text, against what the model
(tests/overdispersion_model.py, format_files) makes of the records the host library parses and of the panel's error table: the text
columns, the counts and the verdicts exactly, the numeric columns parsed and held to the tolerances of tests/test_gpu_overdispersion.py
(Q 1e-5, omega its forward bound, X2 and z dispersion's 1e-12) plus half a unit of the last printed digit.  The cohort has ten positions
listed twice (their second lines with other counts), a header-only file among the tumours and reference bases that are N and lower
case.  Several chunks on both sides: the stream gives a chunk max(AMPLISOLVE_CHUNK_BYTES / (P * 16), min(files, AMPLISOLVE_THREADS))
files of uint16 records; with P = 200, 7000 bytes and 2 threads that is max(2, 2) = 2 files, so the 32 normals are 16 resident chunks
and the 5 tumours 3 streamed ones -- the command says how many it saw, and the test reads that."""
import os
import subprocess

import numpy as np
import pytest

from amplisolve_amd.hostio import HostCohort
from tests.dispersion_model import dispersion_model
from tests.overdispersion_cohorts import planted
from tests.overdispersion_model import NA, format_files, omega_model, s2_model, score_model
from tests.test_gpu_overdispersion import _chunks

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "amplisolve_amd", "bin", "AmpliSolveOverdispersedCalling")
HEADER = "chr\tpos\tdbsnp\tMAF\tref\talt\tA\tC\tG\tT\tRD\tArs\tCrs\tGrs\tTrs\n"
FILES = ["Overdispersed_Calls.txt", "Overdispersed_Cells.txt", "Overdispersed_Samples.txt", "Overdispersed_Summary.txt"]
PARAMS = dict(C_value=0.002, coverage_cutoff=100, calling_cutoff=100, z_cutoff=4.0, q_min=13.0)
KEYS = ["C_value", "coverage_cutoff", "calling_cutoff", "z_cutoff", "q_min"]
TWICE, P0, START = 10, 200, 1000


def _write(d):
    normals, tumours, ref, over, variants = planted(P=P0, S=32, T=4)
    P = normals.shape[1]
    bases = ["ACGT"[r] for r in ref]
    bases[5], bases[17] = "N", bases[17].lower()
    again = list(range(P - TWICE, P))
    (d / "p.bed").write_text(f"chr7\t{START}\t{START + P - 1}\nchr7\t{START + P - TWICE}\t{START + P - 1}\n")
    walk = list(range(P)) + again
    (d / "r.txt").write_text("".join(f"chr7\t{START + p}\t{bases[p]}\n" for p in walk))
    for sub in ("N", "T"):
        (d / sub).mkdir()
    for sub, recs, stem in (("N", normals, "NORM"), ("T", tumours, "TUM")):
        for s in range(recs.shape[0]):
            seen, text = set(), HEADER
            for p in walk:
                r = recs[s, p if p not in seen else (p + 7) % P].astype(np.int64)  # the second line of a position: other counts
                seen.add(p)
                tot = r[:4] + r[4:]
                text += f"chr7\t{START + p}\t.\t.\t.\t.\t{tot[0]}\t{tot[1]}\t{tot[2]}\t{tot[3]}\t{tot.sum()}\t{r[4]}\t{r[5]}\t{r[6]}\t{r[7]}\n"
            (d / sub / f"{stem}{s:02d}.PILEUP.ASEQ").write_text(text)
    (d / "T" / "TNONE.PILEUP.ASEQ").write_text(HEADER)
    return bases


def _run(args, cwd, **env):
    e = dict(os.environ, **env)
    e.pop("AMPLISOLVE_LIST_DIR_AS", None)
    return subprocess.run([EXE] + args, capture_output=True, text=True, cwd=cwd, env=e)


def _args(d, out, **kw):
    p = dict(PARAMS, **kw)
    return [f"panel_design={d / 'p.bed'}", "reference_genome=unused.fa", f"germline_dir={d / 'N'}", f"tumour_dir={d / 'T'}"] + [f"{k}={p[k]}" for k in KEYS] + [
        f"output_dir={d / out}"]


def _model(ctx, d, bases):
    from tests.test_gpu_parity import _t

    normals = HostCohort(str(d / "p.bed"), str(d / "N"), refbases_file=str(d / "r.txt"))
    tumours = HostCohort(str(d / "p.bed"), str(d / "T"), refbases_file=str(d / "r.txt"))
    P, E = normals.P, normals.E
    assert P == P0 and E == TWICE and tumours.S == 5 and normals.S == 32
    ref = normals.ref_code.copy()
    assert ref[5] == 255 and ref[17] == 255 and (ref <= 3).sum() == P - 2
    cov = PARAMS["coverage_cutoff"]
    # the panel's own table, from the project's error estimation over the records as parsed (the extras included)
    rec = _chunks(ctx, normals.recs, P, E, normals.dup_off, normals.ext_pos, None, "i32", (0, normals.S))[0]
    table = ctx.error_reduce_records(rec, P, ctx.new_acc(P), PARAMS["C_value"], cov, finalize=True)
    thr = table.thr.cpu().numpy().reshape(2, 4, P)
    disp = dispersion_model(normals.recs, P, cov, E=E, ext_pos=normals.ext_pos, z_cutoff=PARAMS["z_cutoff"])
    s2 = s2_model(normals.recs, P, cov, E=E, ext_pos=normals.ext_pos)
    omega, bound = omega_model(disp["status"], disp["n"], disp["K"], disp["D"], disp["x2"], s2)
    q0, _ = score_model(tumours.recs, P, thr, None, ref, PARAMS["calling_cutoff"])
    q, q64 = score_model(tumours.recs, P, thr, omega, ref, PARAMS["calling_cutoff"])
    ev = q0 != NA
    assert not (ev & (np.abs(q64 - PARAMS["q_min"]) <= 1e-3)).any()  # no score of this cohort sits where a verdict could turn
    positions = [("chr7", START + p) for p in range(P)]
    return format_files(tumours.names, normals.S, positions, bases, np.where(ref <= 3, ref, 0), tumours.recs, q0, q, omega, disp, PARAMS), bound


TEXT = {"Overdispersed_Calls.txt": (0, 1, 2, 3, 4, 5, 6, 7, 14), "Overdispersed_Cells.txt": (0, 1, 2, 3, 4, 5, 6, 7)}
TOL = {"Overdispersed_Calls.txt": {8: 6e-5, 9: 6e-5, 10: 1e-5, 11: 1e-5, 12: 6e-5, 13: 6e-5}, "Overdispersed_Cells.txt": {8: 1e-6, 9: 1e-4, 10: 1e-5}}


def _same(d, out, exp):
    assert sorted(os.listdir(d / out)) == FILES
    for name in ("Overdispersed_Samples.txt", "Overdispersed_Summary.txt"):
        assert (d / out / name).read_text() == exp[name], name
    for name in TEXT:
        got, want = (d / out / name).read_text().split("\n"), exp[name].split("\n")
        assert len(got) == len(want) and got[0] == want[0] and got[-1] == want[-1] == "", name
        for g, w in zip(got[1:-1], want[1:-1]):
            g, w = g.split("\t"), w.split("\t")
            assert len(g) == len(w) and all(g[c] == w[c] for c in TEXT[name]), (name, g, w)
            for c, tol in TOL[name].items():  # Q to 1e-5 and half a unit of %.4f; omega, X2 and z relative to the printed six digits
                a, b = float(g[c]), float(w[c])
                assert abs(a - b) <= (tol if tol >= 6e-5 else tol * max(1.0, abs(b)) * 2), (name, c, g, w)


def test_files_equal_the_model(ctx, tmp_path, monkeypatch):
    d = tmp_path
    monkeypatch.delenv("AMPLISOLVE_LIST_DIR_AS", raising=False)
    bases = _write(d)
    env = dict(AMPLISOLVE_REFBASES_FILE=str(d / "r.txt"))
    exp, _ = _model(ctx, d, bases)
    calls, summary = exp["Overdispersed_Calls.txt"], exp["Overdispersed_Summary.txt"]
    print(summary)
    assert "normals=32\ntumours=5\npositions=200\n" in summary and "TNONE\t0\t0\t0\t0\n" in exp["Overdispersed_Samples.txt"]
    assert calls.count("\tKEPT\n") >= 16 and calls.count("\tDROPPED\n") >= 3 and "\ndropped=0\n" not in summary
    r = _run(_args(d, "one"), d, **env)
    assert r.returncode == 0, r.stdout[-800:] + r.stderr[-300:]
    assert "5 tumours in 1 chunks against 32 normals in 1 chunks" in r.stdout, r.stdout[-400:]
    _same(d, "one", exp)
    r = _run(_args(d, "chunks"), d, AMPLISOLVE_CHUNK_BYTES="7000", AMPLISOLVE_THREADS="2", **env)  # two files per chunk: the same files
    assert r.returncode == 0, r.stdout[-800:] + r.stderr[-300:]
    assert "5 tumours in 3 chunks against 32 normals in 16 chunks" in r.stdout, r.stdout[-400:]
    _same(d, "chunks", exp)  # X2 is added up chunk by chunk, so the two runs agree within the tolerances, not byte for byte


def test_exit_status_and_refusals(tmp_path):
    d = tmp_path
    _write(d)
    env = dict(AMPLISOLVE_REFBASES_FILE=str(d / "r.txt"))
    for k, v in (("germline_dir", "no_such_dir"), ("tumour_dir", "no_such_dir")):
        a = [f"{k}={d / v}" if x.startswith(k + "=") else x for x in _args(d, "o")]
        r = _run(a, d, **env)
        assert r.returncode == 1 and "failed" in r.stdout and not os.path.exists(d / "o"), k
    r = _run(_args(d, "o"), d, AMPLISOLVE_REFBASES_FILE=str(d / "none.txt"))
    assert r.returncode == 1 and "failed" in r.stdout and not os.path.exists(d / "o")
    r = _run(_args(d, "o", q_min=5, z_cutoff=-50, calling_cutoff=0, coverage_cutoff=1), d, **env)
    assert r.returncode == 0 and sorted(os.listdir(d / "o")) == FILES
