"""AmpliSolveContamination on the planted cohort (tests/contamination_cohorts.py) written as ASEQ text over a panel of two overlapping
amplicons (ten positions listed twice, their second lines with other counts), with a header-only file among the normals: its three
files, byte for byte, against what the model (tests/contamination_model.py) formats from the records the host library parses; the same
bytes from several chunks; every file in the germline directory with tumour_dir=- and other thresholds; and what it refuses."""
import os
import subprocess

import numpy as np
import pytest

from amplisolve_amd.hostio import HostCohort
from tests.concordance_model import classify
from tests.contamination_cohorts import MIXTURES, planted
from tests.contamination_model import format_files, sums

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "amplisolve_amd", "bin", "AmpliSolveContamination")
HEADER = "chr\tpos\tdbsnp\tMAF\tref\talt\tA\tC\tG\tT\tRD\tArs\tCrs\tGrs\tTrs\n"
FILES = ["Contamination_Pairs.txt", "Contamination_Samples.txt", "Contamination_Summary.txt"]
NAMES = [f"I{i}" for i in range(6)] + [f"M{k}" for k in range(len(MIXTURES))]


def _write(d):
    """p.bed / r.txt and N (the six clean samples and a header-only file), T (the six mixtures), ALL (the twelve)"""
    recs, _ = planted()
    P = recs.shape[1]
    rows = [("chr1", 1000, 1000 + P // 2 + 9), ("chr1", 1000 + P // 2, 1000 + P - 1)]  # ten positions in both amplicons
    walk = [x for _, a, b in rows for x in range(a, b + 1)]
    assert len(walk) == P + 10 and len(set(walk)) == P
    (d / "p.bed").write_text("".join(f"{c}\t{a}\t{b}\tAMPL{i}\trs{i}\tGENE{i}\n" for i, (c, a, b) in enumerate(rows)))
    (d / "r.txt").write_text("".join(f"chr1\t{x}\tA\n" for x in walk))
    for sub in ("N", "T", "ALL"):
        (d / sub).mkdir()
    for s, name in enumerate(NAMES):
        seen, text = set(), HEADER
        for x in walk:
            r = recs[s, x - 1000 if x not in seen else (x - 1000 + 7) % P].astype(np.int64)  # the second line of a position: other counts
            seen.add(x)
            tot = r[:4] + r[4:]
            text += f"chr1\t{x}\t.\t.\t.\t.\t{tot[0]}\t{tot[1]}\t{tot[2]}\t{tot[3]}\t{tot.sum()}\t{r[4]}\t{r[5]}\t{r[6]}\t{r[7]}\n"
        for sub in ("N" if s < 6 else "T", "ALL"):
            (d / sub / f"{name}.PILEUP.ASEQ").write_text(text)
    (d / "N" / "EMPTY.PILEUP.ASEQ").write_text(HEADER)


def _run(args, cwd, **env):
    e = dict(os.environ, **env)
    e.pop("AMPLISOLVE_LIST_DIR_AS", None)
    return subprocess.run([EXE] + args, capture_output=True, text=True, cwd=cwd, env=e)


def _args(d, out, germline="N", tumour="T", min_depth=100, min_sites=20, min_fraction="0.005"):
    return [f"panel_design={d / 'p.bed'}", f"germline_dir={d / germline}", f"tumour_dir={d / tumour if tumour != '-' else '-'}",
            f"output_dir={d / out}", f"min_depth={min_depth}", f"min_sites={min_sites}", f"min_fraction={min_fraction}"]


def _model(d, dirs, min_depth, min_sites, min_fraction):
    """the three files from the records as the host library loads them: the directory strings are the command's, so is the visit order"""
    cohorts = [HostCohort(str(d / "p.bed"), str(d / x), refbases_file=str(d / "r.txt")) for x in dirs]
    P = cohorts[0].P
    recs = np.concatenate([c.recs[:, :P] for c in cohorts])
    bits = classify(recs, min_depth=min_depth)
    names = [n for c in cohorts for n in c.names]
    return format_files(names, cohorts[0].S, sums(recs, bits, bits), min_sites, min_fraction, dict(min_depth=min_depth)), cohorts


def _same(d, out, exp):
    assert sorted(os.listdir(d / out)) == FILES
    for name, want in zip(("Contamination_Samples.txt", "Contamination_Pairs.txt", "Contamination_Summary.txt"), exp):
        assert (d / out / name).read_bytes() == want.encode(), name


def test_files_equal_the_model_byte_for_byte(tmp_path, monkeypatch):
    d = tmp_path
    monkeypatch.delenv("AMPLISOLVE_LIST_DIR_AS", raising=False)
    _write(d)
    exp, cohorts = _model(d, ("N", "T"), 100, 20, 0.005)
    recs, _ = planted()
    assert cohorts[0].E == 10 and cohorts[0].S == 7 and cohorts[1].S == 6 and cohorts[0].P == recs.shape[1]
    for c in cohorts:  # the primary records are the planted ones, whatever the order the files are visited in
        for s, name in enumerate(c.names):
            if name != "EMPTY":
                assert np.array_equal(c.recs[s, :c.P], recs[NAMES.index(name)]), name
    rows = {r.split("\t")[0]: r.split("\t") for r in exp[0].splitlines()[1:]}
    assert rows["EMPTY"][1:] == ["N", "0", "0.000000", "NA", "NA", "NA", "NA", "UNDETERMINED"]
    assert rows["M0"][4] == "I1" and rows["M0"][8] == "CONTAMINATED" and rows["M5"][4] == "I2" and rows["M5"][6].startswith("0.15")
    assert rows["M3"][4] == "I0" and rows["M3"][8] == "CLEAN" and rows["I4"][8] == "CLEAN" and rows["M4"][8] == "CLEAN"
    assert "\nM2\tI5\t" in exp[1] and "\nI0\t" not in exp[1] and "normals=7\ntumours=6\n" in exp[2] and "pairs_contaminated=0\n" not in exp[2]
    r = _run(_args(d, "both"), d)
    assert r.returncode == 0, r.stdout[-800:] + r.stderr[-300:]
    _same(d, "both", exp)
    r = _run(_args(d, "chunks"), d, AMPLISOLVE_CHUNK_BYTES="80000")  # the same bytes from several chunks
    assert r.returncode == 0, r.stdout[-800:] + r.stderr[-300:]
    _same(d, "chunks", exp)
    # every file among the normals, no tumours, other thresholds
    exp_n, _ = _model(d, ("ALL",), 30, 5, 0.02)
    r = _run(_args(d, "all", germline="ALL", tumour="-", min_depth=30, min_sites=5, min_fraction="0.02"), d)
    assert r.returncode == 0, r.stdout[-800:] + r.stderr[-300:]
    _same(d, "all", exp_n)
    assert "normals=12\ntumours=0\nmin_depth=30\n" in exp_n[2] and "min_fraction=0.02\n" in exp_n[2] and "\tT\t" not in exp_n[0]
    assert "\nM0\tI1\t" not in exp_n[1] and "\nM1\tI3\t" in exp_n[1]  # 1 % is below this run's min_fraction, 3 % is not


def test_exit_status_and_refusals(tmp_path):
    d = tmp_path
    _write(d)
    r = _run(_args(d, "o", germline="no_such_dir", tumour="-"), d)
    assert r.returncode == 1 and "failed" in r.stdout and "no_such_dir" in r.stdout and not os.path.exists(d / "o")
    r = _run(_args(d, "o", tumour="no_such_dir"), d)
    assert r.returncode == 1 and "failed" in r.stdout and not os.path.exists(d / "o")
    for bad in ("", "0.01x", "nan", "0", "-0.5", "1.5"):
        r = _run(_args(d, "o", tumour="-", min_fraction=bad), d)
        assert r.returncode == 1 and "failed" in r.stdout and "min_fraction" in r.stdout and not os.path.exists(d / "o"), bad
    for key, bad in (("min_depth", "0"), ("min_depth", "x"), ("min_sites", "0"), ("min_sites", "2.5")):
        r = _run(_args(d, "o", tumour="-", **{key: bad}), d)
        assert r.returncode == 1 and "failed" in r.stdout and key in r.stdout and not os.path.exists(d / "o"), (key, bad)
    r = _run(_args(d, "o", tumour="-")[:5], d)
    assert r.returncode == 1 and "Usage" in r.stdout
    r = _run(_args(d, "o", tumour="-"), d, AMPLISOLVE_WORLD_SIZE="2")
    assert r.returncode == 1 and "one GPU" in r.stdout and not os.path.exists(d / "o")
    r = _run(_args(d, "o", tumour="-"), d)
    assert r.returncode == 0 and sorted(os.listdir(d / "o")) == FILES
