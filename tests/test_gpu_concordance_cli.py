"""AmpliSolveSampleConcordance on a fresh panel (overlapping amplicons, so positions listed twice; a header-only file; a tumour's
counts filed a second time among the normals): its three files, byte for byte, against what the model (tests/concordance_model.py)
formats from the records the host library parses; normals only with tumour_dir=-; several chunks; and what it refuses."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from amplisolve_amd.hostio import HostCohort
from tests.concordance_model import classify, format_files, pair_counts
from tests.helpers import write_fresh_panel, write_fresh_tumours

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "amplisolve_amd", "bin", "AmpliSolveSampleConcordance")
HEADER = "chr\tpos\tdbsnp\tMAF\tref\talt\tA\tC\tG\tT\tRD\tArs\tCrs\tGrs\tTrs\n"
FILES = ["Concordance_Pairs.txt", "Concordance_Samples.txt", "Concordance_Summary.txt"]


def _run(args, cwd, **env):
    e = dict(os.environ, **env)
    e.pop("AMPLISOLVE_LIST_DIR_AS", None)
    return subprocess.run([EXE] + args, capture_output=True, text=True, cwd=cwd, env=e)


def _args(d, out, germline="N", tumour="T", min_depth=100, min_sites=5, same_fraction="0.8"):
    return [f"panel_design={d / 'p.bed'}", f"germline_dir={d / germline}", f"tumour_dir={d / tumour if tumour != '-' else '-'}",
            f"min_depth={min_depth}", f"min_sites={min_sites}", f"same_fraction={same_fraction}", f"output_dir={d / out}"]


def _model(d, dirs, min_depth, min_sites, same_fraction):
    """the three files from the records as the host library loads them: the directory strings are the command's, so is the visit order"""
    cohorts = [HostCohort(str(d / "p.bed"), str(d / x), refbases_file=str(d / "r.txt")) for x in dirs]
    P = cohorts[0].P
    bits = classify(np.concatenate([c.recs[:, :P] for c in cohorts]), min_depth=min_depth)
    names = [n for c in cohorts for n in c.names]
    return format_files(names, cohorts[0].S, pair_counts(bits, bits), min_sites, same_fraction, dict(min_depth=min_depth)), cohorts


def _same(d, out, exp):
    assert sorted(os.listdir(d / out)) == FILES
    for name, want in zip(("Concordance_Samples.txt", "Concordance_Pairs.txt", "Concordance_Summary.txt"), exp):
        assert (d / out / name).read_bytes() == want.encode(), name


def test_files_equal_the_model_byte_for_byte(tmp_path, monkeypatch):
    d = tmp_path
    monkeypatch.delenv("AMPLISOLVE_LIST_DIR_AS", raising=False)
    assert write_fresh_panel(d, 141, depth=2000, S=6) > 0          # positions listed twice
    write_fresh_tumours(d, 141, T=3, depth=2000)
    shutil.copy(d / "T" / "K02.PILEUP.ASEQ", d / "N" / "K02N.PILEUP.ASEQ")  # a patient's own normal, here: the same counts, in the panel
    (d / "N" / "EMPTY.PILEUP.ASEQ").write_text(HEADER)               # a header-only file: no valid site, no partner
    exp, cohorts = _model(d, ("N", "T"), 100, 5, 0.8)
    assert cohorts[0].E > 0 and cohorts[0].S == 8 and cohorts[1].S == 3
    assert "K02N\tK02\t" in exp[1] and "\tSAME\n" in exp[1] and "\tUNDETERMINED\n" in exp[1] and "EMPTY\tN\t0\t0\t0\tNA\tNA\tNA\tNA\n" in exp[0]
    assert "pairs_same=1\n" in exp[2] and "pairs_different=0\n" not in exp[2]
    r = _run(_args(d, "both"), d)
    assert r.returncode == 0, r.stdout[-800:] + r.stderr[-300:]
    _same(d, "both", exp)
    r = _run(_args(d, "chunks"), d, AMPLISOLVE_CHUNK_BYTES="80000")  # the same bytes from several chunks
    assert r.returncode == 0, r.stdout[-800:] + r.stderr[-300:]
    _same(d, "chunks", exp)
    # normals only, other thresholds
    exp_n, _ = _model(d, ("N",), 30, 2, 1.0)
    r = _run(_args(d, "normals", tumour="-", min_depth=30, min_sites=2, same_fraction="1"), d)
    assert r.returncode == 0, r.stdout[-800:] + r.stderr[-300:]
    _same(d, "normals", exp_n)
    assert "tumours=0\n" in exp_n[2] and "\tT\t" not in exp_n[0]


def test_exit_status_and_refusals(tmp_path):
    d = tmp_path
    write_fresh_panel(d, 142, depth=2000, S=3, amplicons=2)
    r = _run(_args(d, "o", germline="no_such_dir", tumour="-"), d)
    assert r.returncode == 1 and "failed" in r.stdout and "no_such_dir" in r.stdout and not os.path.exists(d / "o")
    r = _run(_args(d, "o", tumour="no_such_dir"), d)
    assert r.returncode == 1 and "failed" in r.stdout and not os.path.exists(d / "o")
    for bad in ("", "0.8x", "nan", "0", "-0.5", "1.5"):
        r = _run(_args(d, "o", tumour="-", same_fraction=bad), d)
        assert r.returncode == 1 and "failed" in r.stdout and "same_fraction" in r.stdout and not os.path.exists(d / "o"), bad
    for key, bad in (("min_depth", "0"), ("min_depth", "x"), ("min_sites", "0"), ("min_sites", "2.5")):
        r = _run(_args(d, "o", tumour="-", **{key: bad}), d)
        assert r.returncode == 1 and "failed" in r.stdout and key in r.stdout and not os.path.exists(d / "o"), (key, bad)
    r = _run(_args(d, "o", tumour="-")[:5], d)
    assert r.returncode == 1 and "Usage" in r.stdout
    r = _run(_args(d, "o", tumour="-"), d, AMPLISOLVE_WORLD_SIZE="2")
    assert r.returncode == 1 and not os.path.exists(d / "o")
    r = _run(_args(d, "o", tumour="-"), d)
    assert r.returncode == 0 and sorted(os.listdir(d / "o")) == FILES
