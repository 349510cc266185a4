"""AmpliSolveAmpliconCoverage on the planted cohort (tests/amplicon_cohorts.py) written as ASEQ text: its four files, byte for byte,
against what the model (tests/amplicon_model.py, format_files) makes of the records the host library parses.  The cohort has the
positions two overlapping amplicons share listed twice (their second lines with other counts), a header-only file among the normals,
several chunks (a small AMPLISOLVE_CHUNK_BYTES), a BED with and without the columns 4-6; tumour_dir=- and exclude_chrom=- are covered,
and what the command refuses."""
import os
import subprocess

import numpy as np
import pytest

from amplisolve_amd.hostio import HostCohort
from tests.amplicon_cohorts import CHROMS, GAIN_GENE, LOSS_GENE, PER_GENE, ZERO_AMPLICON, planted
from tests.amplicon_model import ABSENT, bed_lists, depth_sums, format_files, ratios, read_bed, reference

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "amplisolve_amd", "bin", "AmpliSolveAmpliconCoverage")
HEADER = "chr\tpos\tdbsnp\tMAF\tref\talt\tA\tC\tG\tT\tRD\tArs\tCrs\tGrs\tTrs\n"
FILES = ["Amplicon_Genes.txt", "Amplicon_Ratios.txt", "Amplicon_Reference.txt", "Amplicon_Summary.txt"]
NAMES = [f"N{i:02d}" for i in range(12)] + ["TGAIN", "TLOSS", "TBIG", "TDROP", "TMALE"]
USUAL = dict(coverage_cutoff=100, min_normals=5, min_amplicons=3, z_cutoff=3.0, gain_ratio=1.3, loss_ratio=0.7)


def _write(d):
    """p.bed (six columns), p3.bed (three), r.txt and N (the twelve normals and a header-only file), T (the five tumours), ALL"""
    c = planted()
    recs, P = c["recs"], c["P"]
    coord, rows = {}, []  # position p of the cohort -> (chrom, coordinate): every gene on its chromosome, the amplicons 1000 apart
    for a, (lo, n) in enumerate(c["spans"]):
        chrom = CHROMS[a // PER_GENE]
        first = coord[lo][1] if lo in coord else 10000 * (a + 1)
        for k in range(n):
            coord.setdefault(lo + k, (chrom, first + k))
        rows.append((chrom, first, first + n - 1, f"AMP{a:02d}", f"rs{a}", c["gene_of"][a]))
    (d / "p.bed").write_text("".join("\t".join(str(x) for x in r) + "\n" for r in rows))
    (d / "p3.bed").write_text("".join("\t".join(str(x) for x in r[:3]) + "\n" for r in rows))
    walk = [p for lo, n in c["spans"] for p in range(lo, lo + n)]
    assert len(walk) == P + 20 and len(set(walk)) == P
    (d / "r.txt").write_text("".join(f"{coord[p][0]}\t{coord[p][1]}\tA\n" for p in walk))
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
            text += f"{coord[p][0]}\t{coord[p][1]}\t.\t.\t.\t.\t{tot[0]}\t{tot[1]}\t{tot[2]}\t{tot[3]}\t{tot.sum()}\t{r[4]}\t{r[5]}\t{r[6]}\t{r[7]}\n"
        for sub in ("N" if s < 12 else "T", "ALL"):
            (d / sub / f"{name}.PILEUP.ASEQ").write_text(text)
    (d / "N" / "EMPTY.PILEUP.ASEQ").write_text(HEADER)


def _run(args, cwd, **env):
    e = dict(os.environ, **env)
    e.pop("AMPLISOLVE_LIST_DIR_AS", None)
    return subprocess.run([EXE] + args, capture_output=True, text=True, cwd=cwd, env=e)


def _args(d, out, bed="p.bed", germline="N", tumour="T", exclude_chrom="chrX,chrY", **kw):
    p = dict(USUAL, **kw)
    return [f"panel_design={d / bed}", f"germline_dir={d / germline}", f"tumour_dir={d / tumour if tumour != '-' else '-'}", f"output_dir={d / out}",
            f"coverage_cutoff={p['coverage_cutoff']}", f"min_normals={p['min_normals']}", f"min_amplicons={p['min_amplicons']}", f"z_cutoff={p['z_cutoff']}",
            f"gain_ratio={p['gain_ratio']}", f"loss_ratio={p['loss_ratio']}", f"exclude_chrom={exclude_chrom}"]


def _model(d, dirs, bed="p.bed", exclude_chrom="chrX,chrY", **kw):
    """the four files from the records as the host library loads them: the directory strings are the command's, so is the visit order"""
    p = dict(USUAL, **kw)
    cohorts = [HostCohort(str(d / bed), str(d / x), refbases_file=str(d / "r.txt")) for x in dirs]
    rows = read_bed((d / bed).read_text())
    P, walk, dup, off, pos, use = bed_lists(rows, () if exclude_chrom == "-" else exclude_chrom.split(","))
    assert P == cohorts[0].P and len(walk) == cohorts[0].walk_len
    recs = np.concatenate([c.recs[:, :P] for c in cohorts])
    names = [n for c in cohorts for n in c.names]
    sums = depth_sums(recs, off, pos, p["coverage_cutoff"])
    ref = reference(sums[:cohorts[0].S], use, p["min_normals"])
    rat = ratios(sums, use, ref)
    return format_files(names, cohorts[0].S, rows, off, sums, ref, rat, exclude_chrom=exclude_chrom, with_tumours=len(dirs) > 1, **p), cohorts, (off, pos, use)


def _same(d, out, exp):
    assert sorted(os.listdir(d / out)) == FILES
    for name in FILES:
        assert (d / out / name).read_bytes() == exp[name].encode(), name


def test_files_equal_the_model_byte_for_byte(tmp_path, monkeypatch):
    d = tmp_path
    monkeypatch.delenv("AMPLISOLVE_LIST_DIR_AS", raising=False)
    _write(d)
    c = planted()
    exp, cohorts, (off, pos, use) = _model(d, ("N", "T"))
    assert cohorts[0].E == 20 and cohorts[0].S == 13 and cohorts[1].S == 5 and cohorts[0].P == c["P"]
    assert np.array_equal(off, c["amp_off"]) and np.array_equal(pos, c["amp_pos"]) and np.array_equal(use, c["use"])  # the BED's lists are the cohort's
    for co in cohorts:  # the primary records are the planted ones, whatever the order the files are visited in
        for s, name in enumerate(co.names):
            if name != "EMPTY":
                assert np.array_equal(co.recs[s, :co.P], c["recs"][NAMES.index(name)]), name
    genes = exp["Amplicon_Genes.txt"].splitlines()[1:]
    assert sorted(g.split("\t")[0] + g.split("\t")[2] + g.split("\t")[6] for g in genes if not g.split("\t")[2].startswith("X")) == [
        "TGAIN" + GAIN_GENE + "GAIN", "TLOSS" + LOSS_GENE + "LOSS"]
    ref_rows = exp["Amplicon_Reference.txt"].splitlines()[1:]
    assert ref_rows[ZERO_AMPLICON].split("\t")[6] == "DARK" and ref_rows[0].split("\t")[3:5] == ["AMP00", "G0"] and ref_rows[0].split("\t")[7] == "12"
    assert "\nEMPTY\tN\t0\tNA\t0\t40\n" in exp["Amplicon_Summary.txt"] and "normals=13\ntumours=5\namplicons=40\n" in exp["Amplicon_Summary.txt"]
    assert "EMPTY\tN\tAMP00\tG0\t0\t0\t0\t0\tNA\tNA\n" in exp["Amplicon_Ratios.txt"]
    r = _run(_args(d, "both"), d)
    assert r.returncode == 0, r.stdout[-800:] + r.stderr[-300:]
    _same(d, "both", exp)
    r = _run(_args(d, "chunks"), d, AMPLISOLVE_CHUNK_BYTES="700000")  # the same bytes from several chunks
    assert r.returncode == 0, r.stdout[-800:] + r.stderr[-300:]
    _same(d, "chunks", exp)
    # a BED without the columns 4-6: every amplicon is '.', of the one gene '.'; nothing excluded
    exp3, _, (_, _, use3) = _model(d, ("N", "T"), bed="p3.bed", exclude_chrom="-")
    assert use3.all() and "\t.\t.\t" in exp3["Amplicon_Reference.txt"] and "exclude_chrom=-\n" in exp3["Amplicon_Summary.txt"]
    r = _run(_args(d, "three", bed="p3.bed", exclude_chrom="-"), d)
    assert r.returncode == 0, r.stdout[-800:] + r.stderr[-300:]
    _same(d, "three", exp3)
    # every file among the normals, no tumours, other thresholds: every (normal, gene) is listed
    kw = dict(coverage_cutoff=300, min_normals=18, min_amplicons=2, z_cutoff=2.5, gain_ratio=1.2, loss_ratio=0.8)
    exp_n, _, _ = _model(d, ("ALL",), exclude_chrom="chrX", **kw)
    assert exp_n["Amplicon_Genes.txt"].count("\n") == 1 + 17 * 8 and "\tFEW\t17\t" in exp_n["Amplicon_Reference.txt"]
    r = _run(_args(d, "all", germline="ALL", tumour="-", exclude_chrom="chrX", **kw), d)
    assert r.returncode == 0, r.stdout[-800:] + r.stderr[-300:]
    _same(d, "all", exp_n)
    kw["min_normals"] = 17
    exp_n, _, _ = _model(d, ("ALL",), exclude_chrom="chr1,chrX,chr9", **kw)
    assert "\tFEW\t" not in exp_n["Amplicon_Reference.txt"] and "\tLOSS\n" in exp_n["Amplicon_Genes.txt"]
    r = _run(_args(d, "all17", germline="ALL", tumour="-", exclude_chrom="chr1,chrX,chr9", **kw), d)
    assert r.returncode == 0, r.stdout[-800:] + r.stderr[-300:]
    _same(d, "all17", exp_n)


def test_exit_status_and_refusals(tmp_path):
    d = tmp_path
    _write(d)
    r = _run(_args(d, "o", germline="no_such_dir", tumour="-"), d)
    assert r.returncode == 1 and "failed" in r.stdout and "no_such_dir" in r.stdout and not os.path.exists(d / "o")
    r = _run(_args(d, "o", tumour="no_such_dir"), d)
    assert r.returncode == 1 and "failed" in r.stdout and not os.path.exists(d / "o")
    for key, bad in (("coverage_cutoff", "-1"), ("coverage_cutoff", "x"), ("min_normals", "0"), ("min_normals", "2.5"), ("min_amplicons", "0"),
                     ("z_cutoff", "-1"), ("z_cutoff", "nan"), ("z_cutoff", "3x"), ("gain_ratio", "1"), ("gain_ratio", "inf"), ("loss_ratio", "0"),
                     ("loss_ratio", "1"), ("loss_ratio", "")):
        r = _run(_args(d, "o", tumour="-", **{key: bad}), d)
        assert r.returncode == 1 and "failed" in r.stdout and key in r.stdout and not os.path.exists(d / "o"), (key, bad)
    r = _run(_args(d, "o", tumour="-", exclude_chrom=""), d)
    assert r.returncode == 1 and "exclude_chrom" in r.stdout and not os.path.exists(d / "o")
    r = _run(_args(d, "o", tumour="-")[:7], d)
    assert r.returncode == 1 and "Usage" in r.stdout
    r = _run(_args(d, "o", tumour="-"), d, AMPLISOLVE_WORLD_SIZE="2")
    assert r.returncode == 1 and "one GPU" in r.stdout and not os.path.exists(d / "o")
    r = _run(_args(d, "o", tumour="-", coverage_cutoff=0), d)
    assert r.returncode == 0 and sorted(os.listdir(d / "o")) == FILES
