"""AmpliSolveNormalExceedance on the planted cohort (tests/exceedance_cohorts.py) written as ASEQ text: its four files, byte for byte,
against what the model (tests/exceedance_model.py, format_files) makes of the records the host library parses.  The cohort has ten
positions listed twice (an overlapping BED row; their second lines with other counts), a header-only file among the tumours, several
chunks on both sides (a small AMPLISOLVE_CHUNK_BYTES), reference bases that are N and lower case; tumour_dir=-, parameters other than
the usual ones and a panel with fewer normals than min_normals are covered, and what the command refuses."""
import os
import subprocess

import numpy as np
import pytest

from amplisolve_amd.hostio import HostCohort
from tests.exceedance_cohorts import N_NORMALS, NAMES, RUNS, planted
from tests.exceedance_model import ABSENT, exceedance, format_files

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "amplisolve_amd", "bin", "AmpliSolveNormalExceedance")
HEADER = "chr\tpos\tdbsnp\tMAF\tref\talt\tA\tC\tG\tT\tRD\tArs\tCrs\tGrs\tTrs\n"
FILES = ["Exceedance_Candidates.txt", "Exceedance_Positions.txt", "Exceedance_Samples.txt", "Exceedance_Summary.txt"]
USUAL = dict(coverage_cutoff=100, calling_cutoff=100, min_alt_reads=3, min_vaf_pm=0, min_normals=10, max_normals=0)
KEYS = list(USUAL)
TWICE, FEW = 10, 6


def _write(d):
    """p.bed (the runs, and a row that lists the last ten positions of the fourth run again), r.txt and N (the 24 normals), T (the five
    tumours, the last of them header-only), FEW (the first six normals)"""
    c = planted()
    recs, P, pos = c["recs"], c["P"], c["positions"]
    rows, start = [], 0
    for p in range(1, P + 1):
        if p == P or pos[p][0] != pos[p - 1][0] or pos[p][1] != pos[p - 1][1] + 1:
            rows.append((pos[start][0], pos[start][1], pos[p - 1][1], start, p))
            start = p
    assert len(rows) == RUNS
    again = list(range(rows[3][4] - TWICE, rows[3][4]))
    rows.append((rows[3][0], pos[again[0]][1], pos[again[-1]][1], 0, 0))
    (d / "p.bed").write_text("".join(f"{r[0]}\t{r[1]}\t{r[2]}\n" for r in rows))
    walk = list(range(P)) + again
    (d / "r.txt").write_text("".join(f"{pos[p][0]}\t{pos[p][1]}\t{c['bases'][pos[p]]}\n" for p in walk))
    for sub in ("N", "T", "FEW"):
        (d / sub).mkdir()
    for s, name in enumerate(NAMES):
        seen, text = set(), HEADER
        for p in walk:
            r = recs[s, p if p not in seen else (p + 7) % P].astype(np.int64)  # the second line of a position: other counts
            seen.add(p)
            if r[0] == ABSENT or recs[s, p, 0] == ABSENT:  # no line, and no second line where there was no first
                continue
            tot = r[:4] + r[4:]
            text += f"{pos[p][0]}\t{pos[p][1]}\t.\t.\t.\t.\t{tot[0]}\t{tot[1]}\t{tot[2]}\t{tot[3]}\t{tot.sum()}\t{r[4]}\t{r[5]}\t{r[6]}\t{r[7]}\n"
        for sub in (["N"] + (["FEW"] if s < FEW else [])) if s < N_NORMALS else ["T"]:
            (d / sub / f"{name}.PILEUP.ASEQ").write_text(text)
    assert (d / "T" / "TNONE.PILEUP.ASEQ").read_text() == HEADER


def _run(args, cwd, **env):
    e = dict(os.environ, **env)
    e.pop("AMPLISOLVE_LIST_DIR_AS", None)
    return subprocess.run([EXE] + args, capture_output=True, text=True, cwd=cwd, env=e)


def _args(d, out, germline="N", tumour="T", **kw):
    p = dict(USUAL, **kw)
    return [f"panel_design={d / 'p.bed'}", "reference_genome=unused.fa", f"germline_dir={d / germline}", f"tumour_dir={d / tumour if tumour != '-' else '-'}",
            f"output_dir={d / out}"] + [f"{k}={p[k]}" for k in KEYS]


def _model(d, germline, tumour, **kw):
    """the four files from the records as the host library loads them: the directory strings are the command's, so is the visit order"""
    p = dict(USUAL, **kw)
    c = planted()
    normals = HostCohort(str(d / "p.bed"), str(d / germline), refbases_file=str(d / "r.txt"))
    tumours = HostCohort(str(d / "p.bed"), str(d / tumour), refbases_file=str(d / "r.txt")) if tumour != "-" else None
    P = normals.P
    assert P == c["P"] and normals.E == TWICE and [normals.position(q) for q in (0, 1, P - 1)] == [c["positions"][q] for q in (0, 1, P - 1)]
    assert np.array_equal(normals.ref_code, c["ref_code"])  # the host's exact match, as the cohort's: N and the lower-case base are 255
    for co in (normals, tumours) if tumours else (normals,):  # the primary records are the planted ones, whatever the order of the files
        for s, name in enumerate(co.names):
            assert np.array_equal(co.recs[s, :P], c["recs"][NAMES.index(name)]), name
    test = tumours if tumours else normals
    cut = dict(normal_cutoff=p["coverage_cutoff"], calling_cutoff=p["calling_cutoff"])
    if tumours:
        elig, ge = exceedance(test.recs, normals.recs, c["ref_code"], first_t=normals.S, **cut)
    else:
        elig, ge = exceedance(test.recs, normals.recs, c["ref_code"], skip_same_index=True, **cut)
    bases = [c["bases"][q] for q in c["positions"]]
    return format_files(test.names, normals.S, tumours.S if tumours else 0, c["positions"], bases, c["ref_code"], test.recs, elig, ge,
                        skip_same_index=tumours is None, **p)


def _same(d, out, exp):
    assert sorted(os.listdir(d / out)) == FILES
    for name in FILES:
        assert (d / out / name).read_bytes() == exp[name].encode(), name


def test_files_equal_the_model_byte_for_byte(tmp_path, monkeypatch):
    d = tmp_path
    monkeypatch.delenv("AMPLISOLVE_LIST_DIR_AS", raising=False)
    _write(d)
    env = dict(AMPLISOLVE_REFBASES_FILE=str(d / "r.txt"))
    exp = _model(d, "N", "T")
    summary, cand = exp["Exceedance_Summary.txt"], exp["Exceedance_Candidates.txt"]
    assert "normals=24\ntumours=5\n" in summary and "skip_same_index=0\n" in summary and f"positions_with_reference={planted()['P'] - 3}\n" in summary
    assert cand.count("\nTVAR\t") >= 40 and "\nTSHALLOW\t" not in cand and "\nTNONE\t" not in cand and "\t24\t0\t0\n" in cand
    assert "TNONE\t0\t0\t0.0000\n" in exp["Exceedance_Samples.txt"] and "TSHALLOW\t0\t0\t0.0000\n" in exp["Exceedance_Samples.txt"]
    assert "\tN\t" in exp["Exceedance_Positions.txt"] and "\t24.0\t" in exp["Exceedance_Positions.txt"]
    r = _run(_args(d, "both"), d, **env)
    assert r.returncode == 0, r.stdout[-800:] + r.stderr[-300:]
    _same(d, "both", exp)
    r = _run(_args(d, "chunks"), d, AMPLISOLVE_CHUNK_BYTES="150000", **env)  # the same bytes from several chunks on both sides
    assert r.returncode == 0, r.stdout[-800:] + r.stderr[-300:]
    _same(d, "chunks", exp)
    # the normals against themselves, each without its own file
    exp_n = _model(d, "N", "-")
    assert "normals=24\ntumours=0\n" in exp_n["Exceedance_Summary.txt"] and "skip_same_index=1\n" in exp_n["Exceedance_Summary.txt"]
    assert "\t23.0\t" in exp_n["Exceedance_Positions.txt"] and "\t24.0\t" not in exp_n["Exceedance_Positions.txt"]
    for out, extra in (("self", {}), ("self_chunks", dict(AMPLISOLVE_CHUNK_BYTES="150000"))):
        r = _run(_args(d, out, tumour="-"), d, **env, **extra)
        assert r.returncode == 0, r.stdout[-800:] + r.stderr[-300:]
        _same(d, out, exp_n)
    # other parameters
    kw = dict(coverage_cutoff=1500, calling_cutoff=700, min_alt_reads=1, min_vaf_pm=30, min_normals=12, max_normals=2)
    exp_k = _model(d, "N", "T", **kw)
    assert exp_k["Exceedance_Candidates.txt"] != cand and exp_k["Exceedance_Candidates.txt"].count("\nTHET\t") >= 5
    r = _run(_args(d, "other", **kw), d, **env)
    assert r.returncode == 0, r.stdout[-800:] + r.stderr[-300:]
    _same(d, "other", exp_k)
    # a panel with fewer normals than min_normals: every count is there, and no candidate
    exp_f = _model(d, "FEW", "T")
    assert "normals=6\n" in exp_f["Exceedance_Summary.txt"] and "\ncandidates=0\n" in exp_f["Exceedance_Summary.txt"] and "\nevaluated=0\n" not in exp_f["Exceedance_Summary.txt"]
    assert exp_f["Exceedance_Candidates.txt"].count("\n") == 1
    r = _run(_args(d, "few", germline="FEW"), d, **env)
    assert r.returncode == 0, r.stdout[-800:] + r.stderr[-300:]
    _same(d, "few", exp_f)


def test_exit_status_and_refusals(tmp_path):
    d = tmp_path
    _write(d)
    env = dict(AMPLISOLVE_REFBASES_FILE=str(d / "r.txt"))
    r = _run(_args(d, "o", germline="no_such_dir", tumour="-"), d, **env)
    assert r.returncode == 1 and "failed" in r.stdout and "no_such_dir" in r.stdout and not os.path.exists(d / "o")
    r = _run(_args(d, "o", tumour="no_such_dir"), d, **env)
    assert r.returncode == 1 and "failed" in r.stdout and not os.path.exists(d / "o")
    for key, bad in (("coverage_cutoff", "-1"), ("coverage_cutoff", "x"), ("calling_cutoff", "-1"), ("calling_cutoff", "1e2"), ("min_alt_reads", "-1"),
                     ("min_alt_reads", "2.5"), ("min_vaf_pm", "-1"), ("min_vaf_pm", "1001"), ("min_normals", "-1"), ("min_normals", ""), ("max_normals", "-1"),
                     ("max_normals", "65535"), ("max_normals", "3x")):
        r = _run(_args(d, "o", tumour="-", **{key: bad}), d, **env)
        assert r.returncode == 1 and "failed" in r.stdout and key in r.stdout and not os.path.exists(d / "o"), (key, bad)
    r = _run(_args(d, "o", tumour="-")[:7], d, **env)
    assert r.returncode == 1 and "Usage" in r.stdout
    r = _run(_args(d, "o", tumour="-"), d, AMPLISOLVE_WORLD_SIZE="2", **env)
    assert r.returncode == 1 and "one GPU" in r.stdout and not os.path.exists(d / "o")
    r = _run(_args(d, "o", tumour="-"), d, AMPLISOLVE_REFBASES_FILE=str(d / "none.txt"))
    assert r.returncode == 1 and "failed" in r.stdout and not os.path.exists(d / "o")
    r = _run(_args(d, "o", germline="FEW", coverage_cutoff=0, calling_cutoff=0, min_alt_reads=0, min_normals=0, max_normals=65534), d, **env)
    assert r.returncode == 0 and sorted(os.listdir(d / "o")) == FILES
