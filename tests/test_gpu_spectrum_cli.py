"""AmpliSolveSubstitutionSpectrum on the planted cohort (tests/spectrum_cohorts.py) written as ASEQ text: its four files, byte for byte,
against what the model (tests/spectrum_model.py, format_files) makes of the records the host library parses.  The cohort has ten
positions listed twice (an overlapping BED row; their second lines with other counts), a header-only file among the tumours, several
chunks (a small AMPLISOLVE_CHUNK_BYTES), reference bases that are N and lower case; tumour_dir=- is covered, and what the command
refuses."""
import os
import subprocess

import numpy as np
import pytest

from amplisolve_amd.hostio import HostCohort
from tests.spectrum_cohorts import NAMES, N_NORMALS, planted
from tests.spectrum_model import ABSENT, CLASSES, class_sums, fold, format_files, panel_classes, score

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "amplisolve_amd", "bin", "AmpliSolveSubstitutionSpectrum")
HEADER = "chr\tpos\tdbsnp\tMAF\tref\talt\tA\tC\tG\tT\tRD\tArs\tCrs\tGrs\tTrs\n"
FILES = ["Spectrum_Contexts.txt", "Spectrum_Reference.txt", "Spectrum_Samples.txt", "Spectrum_Summary.txt"]
USUAL = dict(coverage_cutoff=100, max_alt_pm=30, min_sites=200, min_normals=5, excess_ratio=3.0, z_cutoff=10.0, asym_delta=0.15)
TWICE = 10


def _write(d):
    """p.bed (the runs, and a row that lists the last ten positions of the fourth run again), r.txt and N (the twelve normals), T (the
    six tumours, the last of them header-only), ALL"""
    c = planted()
    recs, P, pos = c["recs"], c["P"], c["positions"]
    rows, start = [], 0
    for p in range(1, P + 1):
        if p == P or pos[p][0] != pos[p - 1][0] or pos[p][1] != pos[p - 1][1] + 1:
            rows.append((pos[start][0], pos[start][1], pos[p - 1][1], start, p))
            start = p
    assert len(rows) == 24
    again = list(range(rows[3][4] - TWICE, rows[3][4]))
    rows.append((rows[3][0], pos[again[0]][1], pos[again[-1]][1], 0, 0))
    (d / "p.bed").write_text("".join(f"{r[0]}\t{r[1]}\t{r[2]}\n" for r in rows))
    walk = list(range(P)) + again
    (d / "r.txt").write_text("".join(f"{pos[p][0]}\t{pos[p][1]}\t{c['bases'][pos[p]]}\n" for p in walk))
    for sub in ("N", "T", "ALL"):
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
        for sub in ("N" if s < N_NORMALS else "T", "ALL"):
            (d / sub / f"{name}.PILEUP.ASEQ").write_text(text)
    assert (d / "T" / "TNONE.PILEUP.ASEQ").read_text() == HEADER


def _run(args, cwd, **env):
    e = dict(os.environ, **env)
    e.pop("AMPLISOLVE_LIST_DIR_AS", None)
    return subprocess.run([EXE] + args, capture_output=True, text=True, cwd=cwd, env=e)


def _args(d, out, germline="N", tumour="T", **kw):
    p = dict(USUAL, **kw)
    return [f"panel_design={d / 'p.bed'}", "reference_genome=unused.fa", f"germline_dir={d / germline}", f"tumour_dir={d / tumour if tumour != '-' else '-'}",
            f"output_dir={d / out}", f"coverage_cutoff={p['coverage_cutoff']}", f"max_alt_pm={p['max_alt_pm']}", f"min_sites={p['min_sites']}",
            f"min_normals={p['min_normals']}", f"excess_ratio={p['excess_ratio']}", f"z_cutoff={p['z_cutoff']}", f"asym_delta={p['asym_delta']}"]


def _model(d, dirs, **kw):
    """the four files from the records as the host library loads them: the directory strings are the command's, so is the visit order"""
    p = dict(USUAL, **kw)
    c = planted()
    cohorts = [HostCohort(str(d / "p.bed"), str(d / x), refbases_file=str(d / "r.txt")) for x in dirs]
    co = cohorts[0]
    assert co.P == c["P"] and [co.position(q) for q in (0, 1, co.P - 1)] == [c["positions"][q] for q in (0, 1, co.P - 1)]
    ref, cls = panel_classes(c["positions"], c["bases"])
    assert np.array_equal(co.ref_code, ref)  # the host's exact match, as the model's
    recs = np.concatenate([x.recs[:, :co.P] for x in cohorts])
    names = [n for x in cohorts for n in x.names]
    sums = class_sums(recs, ref, cls, CLASSES, p["coverage_cutoff"], p["max_alt_pm"])
    f = fold(sums)
    sc = score(f, co.S, **{k: p[k] for k in ("min_sites", "min_normals", "excess_ratio", "z_cutoff", "asym_delta")})
    return format_files(names, co.S, cls, sums, f, sc, **p), cohorts


def _same(d, out, exp):
    assert sorted(os.listdir(d / out)) == FILES
    for name in FILES:
        assert (d / out / name).read_bytes() == exp[name].encode(), name


def test_files_equal_the_model_byte_for_byte(tmp_path, monkeypatch):
    d = tmp_path
    monkeypatch.delenv("AMPLISOLVE_LIST_DIR_AS", raising=False)
    _write(d)
    c = planted()
    exp, cohorts = _model(d, ("N", "T"))
    assert cohorts[0].E == TWICE and cohorts[0].S == 12 and cohorts[1].S == 6
    for co in cohorts:  # the primary records are the planted ones, whatever the order the files are visited in
        for s, name in enumerate(co.names):
            assert np.array_equal(co.recs[s, :co.P], c["recs"][NAMES.index(name)]), name
    summary = exp["Spectrum_Summary.txt"]
    assert "normals=12\ntumours=6\n" in summary and "positions_skipped=4\n" in summary and "classes_used=68\n" in summary
    assert "\nTDEAM\tT\t" in summary and "\tC>T:ELEVATED,G>A:ELEVATED\n" in summary and "\tG>T:ASYMMETRIC\n" in summary
    assert summary.count("\t-\n") == 14 and "TNONE\tT\t0\t0\t0\t0\tA>C:LOW_SITES," in summary
    assert "TNONE\tT\tALL\t0\t0\t0\t0\t0\tNA\tNA\tNA\tNA\tNA\tLOW_SITES\n" in exp["Spectrum_Samples.txt"]
    assert exp["Spectrum_Contexts.txt"].count("\n") == 1 + 18 * 96 and "TNONE\tT\tA[C>A]A\t0\t0\tNA\n" in exp["Spectrum_Contexts.txt"]
    r = _run(_args(d, "both"), d, AMPLISOLVE_REFBASES_FILE=str(d / "r.txt"))
    assert r.returncode == 0, r.stdout[-800:] + r.stderr[-300:]
    _same(d, "both", exp)
    r = _run(_args(d, "chunks"), d, AMPLISOLVE_REFBASES_FILE=str(d / "r.txt"), AMPLISOLVE_CHUNK_BYTES="300000")  # the same bytes from several chunks
    assert r.returncode == 0, r.stdout[-800:] + r.stderr[-300:]
    _same(d, "chunks", exp)
    # every file among the normals, no tumours, other thresholds
    kw = dict(coverage_cutoff=300, max_alt_pm=10, min_sites=150, min_normals=16, excess_ratio=1.2, z_cutoff=2.5, asym_delta=0.02)
    exp_n, _ = _model(d, ("ALL",), **kw)
    assert "normals=18\ntumours=0\n" in exp_n["Spectrum_Summary.txt"] and "\tT\t" not in exp_n["Spectrum_Samples.txt"]
    assert "ELEVATED" in exp_n["Spectrum_Summary.txt"] and "\t16\t" in exp_n["Spectrum_Reference.txt"]
    r = _run(_args(d, "all", germline="ALL", tumour="-", **kw), d, AMPLISOLVE_REFBASES_FILE=str(d / "r.txt"))
    assert r.returncode == 0, r.stdout[-800:] + r.stderr[-300:]
    _same(d, "all", exp_n)
    kw["min_normals"] = 17
    exp_n, _ = _model(d, ("ALL",), **kw)
    assert "\tFEW\n" in exp_n["Spectrum_Reference.txt"] and "NO_REFERENCE" in exp_n["Spectrum_Samples.txt"]
    r = _run(_args(d, "few", germline="ALL", tumour="-", **kw), d, AMPLISOLVE_REFBASES_FILE=str(d / "r.txt"))
    assert r.returncode == 0, r.stdout[-800:] + r.stderr[-300:]
    _same(d, "few", exp_n)


def test_exit_status_and_refusals(tmp_path):
    d = tmp_path
    _write(d)
    env = dict(AMPLISOLVE_REFBASES_FILE=str(d / "r.txt"))
    r = _run(_args(d, "o", germline="no_such_dir", tumour="-"), d, **env)
    assert r.returncode == 1 and "failed" in r.stdout and "no_such_dir" in r.stdout and not os.path.exists(d / "o")
    r = _run(_args(d, "o", tumour="no_such_dir"), d, **env)
    assert r.returncode == 1 and "failed" in r.stdout and not os.path.exists(d / "o")
    for key, bad in (("coverage_cutoff", "-1"), ("coverage_cutoff", "x"), ("max_alt_pm", "-1"), ("max_alt_pm", "1001"), ("max_alt_pm", "3.5"), ("min_sites", "0"),
                     ("min_normals", "0"), ("min_normals", "2.5"), ("excess_ratio", "1"), ("excess_ratio", "inf"), ("z_cutoff", "-1"), ("z_cutoff", "nan"),
                     ("z_cutoff", "3x"), ("asym_delta", "-0.1"), ("asym_delta", "1.5"), ("asym_delta", "")):
        r = _run(_args(d, "o", tumour="-", **{key: bad}), d, **env)
        assert r.returncode == 1 and "failed" in r.stdout and key in r.stdout and not os.path.exists(d / "o"), (key, bad)
    r = _run(_args(d, "o", tumour="-")[:7], d, **env)
    assert r.returncode == 1 and "Usage" in r.stdout
    r = _run(_args(d, "o", tumour="-"), d, AMPLISOLVE_WORLD_SIZE="2", **env)
    assert r.returncode == 1 and "one GPU" in r.stdout and not os.path.exists(d / "o")
    r = _run(_args(d, "o", tumour="-"), d, AMPLISOLVE_REFBASES_FILE=str(d / "none.txt"))
    assert r.returncode == 1 and "failed" in r.stdout and not os.path.exists(d / "o")
    r = _run(_args(d, "o", tumour="-", coverage_cutoff=0, max_alt_pm=0), d, **env)
    assert r.returncode == 0 and sorted(os.listdir(d / "o")) == FILES
