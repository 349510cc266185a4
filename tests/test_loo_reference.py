"""The leave-one-out check pinned to the reference itself: for every normal s of a fresh panel, the reference's error estimation over
the other S-1 files (oracle/_ref/ee_ref_driver on a directory of symlinks) and its callVariants without Fisher on s alone
(oracle/_ref/AmpliSolveVariantCalling_noFisher).  CPU: the composed model (tests/loo_model.py) gives the reference's rows and the
S-1 table's thresholds.  GPU: AmpliSolveLeaveOneOut's calls file gives them too, in the gate columns, and its Thr_* the table's."""
import os
import subprocess

import numpy as np
import pytest

from amplisolve_amd.hostio import HostCohort
from oracle import pyoracle as orc
from tests.helpers import write_fresh_panel
from tests.loo_model import loo_model
from tests.test_panel_variants_vs_reference import _vary

pytestmark = pytest.mark.skipif(not (os.path.exists(orc.REF_VC_NOFISHER) and os.path.exists(orc.REF_EE_DRIVER)),
                                reason="oracle/_ref is absent (make -C oracle where /root/reference exists)")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "amplisolve_amd", "bin", "AmpliSolveLeaveOneOut")


def _panel(d, seed, what, S):
    rng = np.random.default_rng(seed)
    write_fresh_panel(d, seed, depth=2000, S=S, amplicons=4)
    _vary(d, rng, what, sub="N")
    # a low-level variant in some normals: what the others' tables call
    for k, f in enumerate(sorted(os.listdir(d / "N"))):
        if k % 2:
            continue
        lines = (d / "N" / f).read_text().splitlines()
        for i in range(1 + k, len(lines), 97):
            tok = lines[i].split("\t")
            tok[7], tok[12] = str(int(tok[7]) + 60), str(int(tok[12]) + 30)  # 60 more C reads, 30 of them reverse
            tok[10] = str(int(tok[10]) + 60) if int(tok[10]) == sum(int(t) for t in tok[6:10]) else tok[10]
            lines[i] = "\t".join(tok)
        (d / "N" / f).write_text("\n".join(lines) + "\n")


def _reference(d, s_file, files, C, cov, call_cov, tag):
    """the reference's two steps for held-out file s_file: its Summary rows and its S-1 table as {(chrom, pos): cells}"""
    n1, ns = d / f"{tag}_N", d / f"{tag}_S"
    n1.mkdir()
    ns.mkdir()
    for f in files:
        (ns if f == s_file else n1).joinpath(f).symlink_to(d / "N" / f)
    (d / f"{tag}_o").mkdir()
    r = subprocess.run([orc.REF_EE_DRIVER, "p.bed", "r.txt", "d.txt", f"{tag}_N", repr(C), str(cov), f"{tag}_o"], capture_output=True, text=True, cwd=d)
    assert r.returncode == 0, r.stderr[-400:]
    table = f"{tag}_o/" + [n for n in os.listdir(d / f"{tag}_o") if n.startswith("positionSpecificNoise_")][0]
    r = subprocess.run([orc.REF_VC_NOFISHER, f"errorFile={table}", f"tumour_dir={tag}_S", f"output_dir={tag}_v", f"coverage_cutoff={call_cov}",
                        "p_value=0.05"], capture_output=True, text=True, cwd=d)
    assert r.returncode == 0, r.stdout[-400:]
    rows = [l.split("\t") for l in (d / f"{tag}_v" / "Summary_Variant_Info.txt").read_text().splitlines()[1:]]
    cells = {}
    for l in (d / table).read_text().splitlines()[1:]:
        t = l.split("\t")
        cells[(t[0], t[1])] = t[4:8]
    return rows, cells


def _thr(cell, strand):
    return float(cell.split("_")[strand]) if "_" in cell else float(cell)


CASES = [(61, (), 100, 100), (62, ("bed_twice",), 30, 100), (63, ("aseq_triple",), 100, 30), (64, ("aseq_own_rd",), 100, 1),
         (65, ("bed_twice", "aseq_triple", "aseq_own_rd"), 1, 100)]


@pytest.mark.parametrize("seed,what,cov,call_cov", CASES)
def test_model_equals_the_reference_run_per_normal(tmp_path, monkeypatch, seed, what, cov, call_cov):
    d = tmp_path
    S, C = 5, 0.002
    _panel(d, seed, what, S)
    monkeypatch.chdir(d)
    co = HostCohort("p.bed", "N", refbases_file="r.txt", keep_line_no=True)
    exp = loo_model(co.recs, co.P, co.ref_code, C, cov, call_cov, E=co.E, dup_off=co.dup_off, ext_pos=co.ext_pos, rd=co.rd_plane())
    assert exp["order_sensitive"] == 0
    files = {n: f for f in os.listdir(d / "N") for n in [f.split(".")[0]]}
    rdp = co.rd_plane()
    n_rows = 0
    for s, name in enumerate(co.names):
        fname = next(f for f in os.listdir(d / "N") if f.startswith(name + "."))
        rows, cells = _reference(d, fname, sorted(os.listdir(d / "N")), C, cov, call_cov, f"h{s}")
        want = []
        for _, r in sorted((co.line_no[s, r], r) for r in range(co.P + co.E) if exp["call_mask"][s, r]):
            p = r if r < co.P else co.ext_pos[r - co.P]
            c, x = co.position(p)
            rec = co.recs[s, r].astype(np.int64)
            RD = int(rdp[s, r]) if rdp is not None and rdp[s, r] != np.iinfo(np.int32).min else int(rec.sum())
            for a in range(4):
                if exp["call_mask"][s, r] >> a & 1:
                    want.append(([c, str(x), f"{'ACGT'[co.ref_code[p]]}->{'ACGT'[a]}", str(RD), str(int(rec[:4].sum())), str(int(rec[4:].sum()))],
                                 [str(int(rec[a])), str(int(rec[4 + a]))], exp["q"][s, r, a], (p, a)))
        assert len(rows) == len(want), (name, len(rows), len(want))
        for g, (w6, wk, q, (p, a)) in zip(rows, want):
            assert g[1:7] == w6 and g[8:10] == wk, (g, w6)
            assert abs(float(g[14]) - q[0]) <= 5e-4 * max(1, q[0]) and abs(float(g[15]) - q[1]) <= 5e-4 * max(1, q[1])
            cell = cells[(g[1], g[2])][a]
            assert (_thr(cell, 0), _thr(cell, 1)) == (float(f"{exp['thr_loo'][s, 0, a, p]:f}"), float(f"{exp['thr_loo'][s, 1, a, p]:f}"))
        n_rows += len(rows)
    assert n_rows > 0
    del files


@pytest.mark.gpu
@pytest.mark.parametrize("seed,what,cov,call_cov", CASES + [(66, ("bed_twice",), 100, 100)])
def test_command_line_equals_the_reference_run_per_normal(tmp_path, monkeypatch, seed, what, cov, call_cov):
    d = tmp_path
    S, C = 5, 0.002
    _panel(d, seed, what, S)
    monkeypatch.chdir(d)
    r = subprocess.run([EXE, "panel_design=p.bed", "reference_genome=unused.fa", "germline_dir=N", f"C_value={C},0.004", f"coverage_cutoff={cov}",
                        f"calling_cutoff={call_cov}", "output_dir=loo"], capture_output=True, text=True, cwd=d,
                       env=dict(os.environ, AMPLISOLVE_REFBASES_FILE="r.txt"))
    assert r.returncode == 0, r.stdout[-600:]
    got = [l.split("\t") for l in (d / "loo" / "leaveOneOut_0.0020_calls.txt").read_text().splitlines()[1:]]
    files = sorted(os.listdir(d / "N"))
    n = 0
    for s, fname in enumerate(files):
        rows, cells = _reference(d, fname, files, C, cov, call_cov, f"h{s}")
        mine = [g for g in got if g[0] == rows[0][0]] if rows else [g for g in got if fname.startswith(g[0] + ".")]
        assert len(mine) == len(rows), fname
        for g, w in zip(mine, rows):
            assert g[:7] == w[:7] and g[8:10] == w[8:10], (g, w)
            # the Summary's first row prints 6 digits, every other 4 (VC:1066); ours prints 4 on every row: equal to the printed precision
            for x, y in zip((g[7], g[10], g[11], g[12], g[13]), (w[7], w[10], w[11], w[14], w[15])):
                assert abs(float(x) - float(y)) <= 5e-4 * abs(float(y)) + 1e-12, (g, w)
            a = "ACGT".index(g[3][-1])
            cell = cells[(g[1], g[2])][a]
            assert (float(g[14]), float(g[15])) == (_thr(cell, 0), _thr(cell, 1)), (g, cell)
        n += len(rows)
    assert n > 0
    # positions / samples files agree with the calls file
    pos = [l.split("\t") for l in (d / "loo" / "leaveOneOut_0.0020_positions.txt").read_text().splitlines()[1:]]
    assert sum(int(t[5]) + int(t[6]) + int(t[7]) + int(t[8]) for t in pos) == len(got)
    sam = [l.split("\t") for l in (d / "loo" / "leaveOneOut_0.0020_samples.txt").read_text().splitlines()[1:]]
    assert sum(int(t[2]) for t in sam) == len(got) and sum(int(t[1]) for t in sam) == sum(int(t[4]) for t in pos)
    # a two-value C list gives the files of a single-C run
    r = subprocess.run([EXE, "panel_design=p.bed", "reference_genome=unused.fa", "germline_dir=N", "C_value=0.004", f"coverage_cutoff={cov}",
                        f"calling_cutoff={call_cov}", "output_dir=one"], capture_output=True, text=True, cwd=d,
                       env=dict(os.environ, AMPLISOLVE_REFBASES_FILE="r.txt"))
    assert r.returncode == 0
    for k in ("calls", "positions", "samples"):
        assert (d / "one" / f"leaveOneOut_0.0040_{k}.txt").read_bytes() == (d / "loo" / f"leaveOneOut_0.0040_{k}.txt").read_bytes()


@pytest.mark.gpu
def test_command_line_refusals(tmp_path, monkeypatch):
    from tests.helpers import write_envelope_panel

    d = tmp_path
    write_envelope_panel(d, 5)
    monkeypatch.chdir(d)
    r = subprocess.run([EXE, "panel_design=p.bed", "reference_genome=unused.fa", "germline_dir=N", "C_value=0.002", "coverage_cutoff=1",
                        "calling_cutoff=100", "output_dir=loo"], capture_output=True, text=True, cwd=d,
                       env=dict(os.environ, AMPLISOLVE_REFBASES_FILE="r.txt"))
    assert r.returncode == 1 and "exactness envelope" in r.stdout
    assert not (d / "loo").exists() or not any(n.startswith("leaveOneOut_") for n in os.listdir(d / "loo"))
    r = subprocess.run([EXE, "panel_design=p.bed", "reference_genome=unused.fa", "germline_dir=N", "C_value=0.002", "coverage_cutoff=100",
                        "calling_cutoff=100", "output_dir=w"], capture_output=True, text=True, cwd=d,
                       env=dict(os.environ, AMPLISOLVE_REFBASES_FILE="r.txt", AMPLISOLVE_WORLD_SIZE="2"))
    assert r.returncode == 1 and "AMPLISOLVE_WORLD_SIZE" in r.stdout
