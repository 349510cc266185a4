"""AmpliSolveAllelicImbalance on a planted cohort written as ASEQ text: its four files against what the model (tests/allelic_model.py,
format_files) makes of the records the host library parses -- integer columns and names byte for byte, score-derived columns to the
printed precision +- 1e-5.  The cohort has a position listed twice in the BED (its second line with other counts), a header-only file
among the normals and several chunks (a small AMPLISOLVE_CHUNK_BYTES); pairs=self, a pairs file and tumour_dir=- are covered."""
import os
import subprocess

import numpy as np
import pytest

from amplisolve_amd.hostio import HostCohort
from tests import allelic_cohorts as ac
from tests import allelic_model as am
from tests.concordance_model import classify

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "amplisolve_amd", "bin", "AmpliSolveAllelicImbalance")
HEADER = "chr\tpos\tdbsnp\tMAF\tref\talt\tA\tC\tG\tT\tRD\tArs\tCrs\tGrs\tTrs\n"
FILES = ["Allelic_Genes.txt", "Allelic_Reference.txt", "Allelic_Sites.txt", "Allelic_Summary.txt"]
USUAL = dict(min_depth=100, min_normals=5, site_q=20.0, min_sites=3, q_min=20.0, min_imbalance=0.02)
ABSENT = np.iinfo(np.int32).min


def _write(d):
    """p.bed: the twelve genes of the planted cohort as rows of 50 positions, and a thirteenth row that lists 20 positions of GENE03 again
    under GENE11 (the positions are listed twice per file); N: the 24 normals and a header-only file; T: the six tumours"""
    co = ac.planted()
    rows = [("chr%d" % (1 + g % 3), 1000 * (g + 1), 1000 * (g + 1) + ac.GENE_LEN - 1, f"AMP{g:02d}", f"rs{g}", f"GENE{g:02d}") for g in range(ac.GENES)]
    rows.append(("chr1", 4010, 4029, "AMP12", "rs12", "GENE11"))
    (d / "p.bed").write_text("".join("\t".join(str(x) for x in r) + "\n" for r in rows))
    walk = [(r[0], x) for r in rows for x in range(r[1], r[2] + 1)]
    index = {}
    for k in walk:
        index.setdefault(k, len(index))
    assert len(index) == ac.P and len(walk) == ac.P + 20
    (d / "r.txt").write_text("".join(f"{c}\t{x}\tA\n" for c, x in walk))
    for sub, recs, tag in (("N", co["normals"], "N"), ("T", co["tumours"], "T")):
        (d / sub).mkdir()
        for s in range(len(recs)):
            seen, text = set(), HEADER
            for k in walk:
                p = index[k]
                r = recs[s, p if k not in seen else (p + 7) % ac.P].astype(np.int64)  # the second line of a position: other counts
                seen.add(k)
                tot = r[:4] + r[4:]
                text += f"{k[0]}\t{k[1]}\t.\t.\t.\t.\t{tot[0]}\t{tot[1]}\t{tot[2]}\t{tot[3]}\t{tot.sum()}\t{r[4]}\t{r[5]}\t{r[6]}\t{r[7]}\n"
            (d / sub / f"{tag}{s:02d}.PILEUP.ASEQ").write_text(text)
    (d / "N" / "EMPTY.PILEUP.ASEQ").write_text(HEADER)
    return rows


def _run(args, cwd, **env):
    e = dict(os.environ, **env)
    e.pop("AMPLISOLVE_LIST_DIR_AS", None)
    return subprocess.run([EXE] + args, capture_output=True, text=True, cwd=cwd, env=e)


def _args(d, out, tumour="T", pairs="self", **kw):
    p = dict(USUAL, **kw)
    return [f"panel_design={d / 'p.bed'}", f"germline_dir={d / 'N'}", f"tumour_dir={d / tumour if tumour != '-' else '-'}", f"pairs={pairs}", f"output_dir={d / out}",
            f"min_depth={p['min_depth']}", f"min_normals={p['min_normals']}", f"site_q={p['site_q']:g}", f"min_sites={p['min_sites']}", f"q_min={p['q_min']:g}",
            f"min_imbalance={p['min_imbalance']:g}"]


def _model(d, rows, tumour="T", pairs=(), **kw):
    """the four files from the records as the host library loads them: the directory strings are the command's, so is the visit order"""
    prm = dict(USUAL, **kw)
    cn = HostCohort(str(d / "p.bed"), str(d / "N"), refbases_file=str(d / "r.txt"))
    c2 = HostCohort(str(d / "p.bed"), str(d / tumour), refbases_file=str(d / "r.txt")) if tumour != "-" else cn
    positions, reg_names, off, pos = am.bed_regions(rows)
    P = len(positions)
    assert P == cn.P == ac.P
    geno = dict(min_depth=prm["min_depth"])
    bits_n, bits_2 = classify(cn.recs[:, :P], **geno), classify(c2.recs[:, :P], **geno)
    ref = am.reference(cn.recs, bits_n, P, prm["min_depth"])
    row_g = np.arange(cn.S, cn.S + c2.S)
    germline_of = ["self"] * c2.S
    for t, n in pairs:
        row_g[c2.names.index(t)] = cn.names.index(n)
        germline_of[c2.names.index(t)] = n
    q, km, v, code, _ = am.sites(c2.recs, P, np.concatenate([bits_n, bits_2]), row_g, ref, prm["min_depth"], prm["min_normals"], True)
    sums = am.region_sums(q, km, v, code, off, pos, prm["site_q"])
    return am.format_files(cn.names, c2.names, germline_of, positions, reg_names, ref, q, km, v, code, sums, prm, tumour != "-", len(pairs)), sums


def _close(d, out, exp):
    """names and integer columns byte for byte; a column printed with decimals to its printed precision +- 1e-5"""
    assert sorted(os.listdir(d / out)) == FILES
    for name in FILES:
        got, want = (d / out / name).read_text().split("\n"), exp[name].split("\n")
        assert len(got) == len(want), name
        for lg, lw in zip(got, want):
            cg, cw = lg.split("\t"), lw.split("\t")
            assert len(cg) == len(cw), (name, lg, lw)
            for col, (a, b) in enumerate(zip(cg, cw)):
                if a != b and name == "Allelic_Genes.txt" and col == 6:
                    # Q20 is the sum of the sites' |q| in units of 2^-20: score-derived, S_TOL = 1e-5 per site
                    assert abs(int(a) - int(b)) <= int(cw[2]) * 1e-5 * (1 << 20), (name, lg, lw)
                elif a != b:
                    assert "." in a and "." in b and len(a.split(".")[1]) == len(b.split(".")[1]), (name, lg, lw)
                    assert abs(float(a) - float(b)) <= 10.0 ** -len(a.split(".")[1]) + 1e-5, (name, lg, lw)


def test_files_equal_the_model(tmp_path, monkeypatch):
    d = tmp_path
    monkeypatch.delenv("AMPLISOLVE_LIST_DIR_AS", raising=False)
    rows = _write(d)
    co = ac.planted()
    exp, sums = _model(d, rows)
    t, g = co["plant"]
    genes = exp["Allelic_Genes.txt"].splitlines()[1:]
    assert [x.split("\t")[:2] for x in genes if x.split("\t")[9] == "IMBALANCED"] == [[f"T{t:02d}", f"GENE{g:02d}"]]  # the planted gene and nothing else
    assert len(genes) == 6 * 13 and "normals=25\nfiles=6\nmode=tumours\npairs=0\npositions=600\nregions=13\n" in exp["Allelic_Summary.txt"]
    assert (sums[:, :, am.SITES] >= 3).mean() > 0.9 and exp["Allelic_Sites.txt"].count("\n") > 300
    r = _run(_args(d, "self"), d)
    assert r.returncode == 0, r.stdout[-800:] + r.stderr[-300:]
    _close(d, "self", exp)
    r = _run(_args(d, "chunks"), d, AMPLISOLVE_CHUNK_BYTES="300000")  # the same files from several chunks
    assert r.returncode == 0, r.stdout[-800:] + r.stderr[-300:]
    _close(d, "chunks", exp)
    for name in FILES:  # the same kernels on the same records: the chunks change no byte
        assert (d / "chunks" / name).read_bytes() == (d / "self" / name).read_bytes()
    # a pairs file: two tumours take a normal's genotype, the others their own; other thresholds
    pairs = [("T02", "N05"), ("T04", "N00")]
    (d / "pairs.txt").write_text("".join(f"{a}\t{b}\n" for a, b in pairs))
    kw = dict(min_depth=300, min_normals=8, site_q=13.0, min_sites=2, q_min=13.0, min_imbalance=0.01)
    exp_p, _ = _model(d, rows, pairs=pairs, **kw)
    assert "T02\tN05\n" in exp_p["Allelic_Summary.txt"] and "T03\tself\n" in exp_p["Allelic_Summary.txt"] and "pairs=2\n" in exp_p["Allelic_Summary.txt"]
    r = _run(_args(d, "pairs", pairs=str(d / "pairs.txt"), **kw), d)
    assert r.returncode == 0, r.stdout[-800:] + r.stderr[-300:]
    _close(d, "pairs", exp_p)
    # the null calibration: the normals again, the header-only file among them
    exp_n, _ = _model(d, rows, tumour="-")
    assert "mode=null_calibration\n" in exp_n["Allelic_Summary.txt"] and "regions_imbalanced=0\n" in exp_n["Allelic_Summary.txt"]
    assert "EMPTY\tALL\t0\t0\t0\t0\t0\tNA\tNA\tFEW\tNA\tNA\n" in exp_n["Allelic_Genes.txt"]
    r = _run(_args(d, "null", tumour="-"), d, AMPLISOLVE_CHUNK_BYTES="300000")
    assert r.returncode == 0, r.stdout[-800:] + r.stderr[-300:]
    _close(d, "null", exp_n)


def test_exit_status(tmp_path):
    d = tmp_path
    _write(d)
    r = _run(_args(d, "o", tumour="no_such_dir"), d)
    assert r.returncode == 1 and "failed" in r.stdout and not os.path.exists(d / "o")
    (d / "Z").mkdir()
    r = _run(_args(d, "o", tumour="Z"), d)
    assert r.returncode == 1 and "no *.ASEQ files" in r.stdout and not os.path.exists(d / "o")
