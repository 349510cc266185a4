"""The planted cohort of the paired comparison (tests/paired_cohorts.py) through Context.pair_score and through
AmpliSolvePairedComparison, against what the model (tests/paired_model.py, format_files) makes of the same records.

Through the command line the cohort is written as ASEQ text into one directory: ten positions listed twice (their second lines with
other counts, which may not matter: only the primary record enters), a header-only file that one pair names, and reference bases that
are N and lower case.  The text columns, the counts and the verdicts are held exactly, S to 1e-5 plus half a unit of %.4f.  Several
resident chunks: the stream gives a chunk max(AMPLISOLVE_CHUNK_BYTES / (P * 16), min(files, AMPLISOLVE_THREADS)) files of uint16
records; with P = 200, 7000 bytes and 2 threads that is 2 files, so the 10 files are 5 chunks and most pairs span two of them -- the
command says how many it saw, and the test reads that.

Required of the device, as measured on the model first (tests/paired_cohorts.py): every planted somatic variant HIGHER_IN_A against
the normal, every germline site SHARED in every pair, background cells called to either side at most twice the model's count.
Verdicts are exact outside a band of 2e-5 around +-q_min, and the band holds no cell of these inputs (checked here on the model)."""
import os
import subprocess

import numpy as np
import pytest

from amplisolve_amd.hostio import HostCohort
from tests.paired_cohorts import CUTOFF, MIN_VAF, P0, Q_MIN, names, pair_names, planted, tally
from tests.paired_model import NA, format_files, score_model
from tests.test_gpu_parity import _t

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "amplisolve_amd", "bin", "AmpliSolvePairedComparison")
HEADER = "chr\tpos\tdbsnp\tMAF\tref\talt\tA\tC\tG\tT\tRD\tArs\tCrs\tGrs\tTrs\n"
FILES = ["Paired_Cells.txt", "Paired_Pairs.txt", "Paired_Summary.txt"]
PARAMS = dict(depth_cutoff=CUTOFF, q_min=Q_MIN, min_vaf=MIN_VAF)
TWICE, START = 10, 1000
S_COLS, VERDICT_COL = (15, 16), 17


def test_planted_cohort_through_context(ctx):
    recs, ref, sites = planted()
    idx = {nm: i for i, nm in enumerate(names())}
    pairs = [(idx[a], idx[b]) for a, b in pair_names()]
    want, want64 = score_model(recs, recs, P0, pairs, ref, CUTOFF)
    ev = want != NA
    assert not (ev & (np.abs(np.abs(want64) - Q_MIN) <= 2e-5)).any()  # the band around +-q_min holds no cell: the verdicts are exact
    r = ctx.records(ctx.pack(_t(recs), "u16")[0], "u16", recs.shape[0])
    got = ctx.pair_score(r, r, P0, _t(np.array(pairs, np.int32)), _t(ref), CUTOFF).cpu().numpy()
    assert np.array_equal(got == NA, ~ev) and (np.abs(got.astype(np.float64) - want64)[ev] <= 1e-5).all()
    tm, tg = tally(want, pairs, sites), tally(got, pairs, sites)
    print("model ", tm)
    print("device", tg)
    # the model's counts, measured before this test was written (tests/paired_cohorts.py)
    assert tm["background"] == (8, 3) and tm["somatic_fall:T_N"] == (9, 0, 9) and tm["somatic_gone:T_N"] == (9, 0, 9) and tm["lost:T_N"] == (0, 3, 3)
    for kind in ("somatic_fall", "somatic_gone"):
        assert tg[f"{kind}:T_N"] == (9, 0, 9) and tg[f"{kind}:F_T"] == (0, 9, 9)          # every planted somatic variant, against the normal
    for kind in ("het", "hom"):
        assert all(tg[f"{kind}:{role}"][:2] == (0, 0) for role in ("T_N", "F_T", "F_N"))  # no germline site to either side
    assert tg["lost:T_N"] == (0, 3, 3) and tg["somatic_fall:F_N"] == (9, 0, 9) and tg["somatic_gone:F_N"] == (0, 0, 9)
    assert tg["background"][0] <= 2 * tm["background"][0] and tg["background"][1] <= 2 * tm["background"][1]
    assert tg == tm  # outside the band the verdicts are exact


def _write(d):
    recs, ref, sites = planted()
    P = recs.shape[1]
    used = {p for lst in sites.values() for _, p, _ in lst}
    free = [p for p in range(P - TWICE) if p not in used]
    bases = ["ACGT"[r] for r in ref]
    bases[free[0]], bases[free[1]] = "N", bases[free[1]].lower()
    again = list(range(P - TWICE, P))
    (d / "p.bed").write_text(f"chr7\t{START}\t{START + P - 1}\nchr7\t{START + P - TWICE}\t{START + P - 1}\n")
    walk = list(range(P)) + again
    (d / "r.txt").write_text("".join(f"chr7\t{START + p}\t{bases[p]}\n" for p in walk))
    (d / "S").mkdir()
    for s, name in enumerate(names()):
        seen, text = set(), HEADER
        for p in walk:
            r = recs[s, p if p not in seen else (p + 7) % P].astype(np.int64)  # the second line of a position: other counts
            seen.add(p)
            tot = r[:4] + r[4:]
            text += f"chr7\t{START + p}\t.\t.\t.\t.\t{tot[0]}\t{tot[1]}\t{tot[2]}\t{tot[3]}\t{tot.sum()}\t{r[4]}\t{r[5]}\t{r[6]}\t{r[7]}\n"
        (d / "S" / f"{name}.PILEUP.ASEQ").write_text(text)
    (d / "S" / "NONE.PILEUP.ASEQ").write_text(HEADER)
    listed = pair_names() + [("P1_T", "NONE")]
    (d / "pairs.txt").write_text("".join(f"{a}\t{b}\n" for a, b in listed))
    return bases, listed, (free[0], free[1])


def _run(args, cwd, **env):
    e = dict(os.environ, **env)
    e.pop("AMPLISOLVE_LIST_DIR_AS", None)
    return subprocess.run([EXE] + args, capture_output=True, text=True, cwd=cwd, env=e, timeout=120)


def _args(d, out, pairs="pairs.txt", **kw):
    p = dict(PARAMS, **kw)
    return [f"panel_design={d / 'p.bed'}", "reference_genome=unused.fa", f"sample_dir={d / 'S'}", f"pairs={d / pairs}", f"depth_cutoff={p['depth_cutoff']}",
            f"q_min={p['q_min']}", f"min_vaf={p['min_vaf']}", f"output_dir={d / out}"]


def _model(d, listed, masked):
    co = HostCohort(str(d / "p.bed"), str(d / "S"), refbases_file=str(d / "r.txt"))
    P = co.P
    assert P == P0 and co.E == TWICE and co.S == 10 and sorted(co.names) == sorted(names() + ["NONE"])
    ref = co.ref_code.copy()
    assert ref[masked[0]] == 255 and ref[masked[1]] == 255 and (ref <= 3).sum() == P - 2
    idx = {nm: i for i, nm in enumerate(co.names)}
    pairs = [(idx[a], idx[b]) for a, b in listed]
    s, s64 = score_model(co.recs, co.recs, P, pairs, ref, CUTOFF)
    assert not ((s != NA) & (np.abs(np.abs(s64) - Q_MIN) <= 1e-3)).any()  # no score of this cohort sits where a verdict could turn
    positions = [("chr7", START + p) for p in range(P)]
    return format_files(co.names, co.names, positions, np.where(ref <= 3, ref, 0), co.recs, co.recs, pairs, s, PARAMS)


def _same(d, out, exp):
    assert sorted(os.listdir(d / out)) == FILES
    for name in ("Paired_Pairs.txt", "Paired_Summary.txt"):
        assert (d / out / name).read_text() == exp[name], name
    got, want = (d / out / "Paired_Cells.txt").read_text().split("\n"), exp["Paired_Cells.txt"].split("\n")
    assert len(got) == len(want) and got[0] == want[0] and got[-1] == want[-1] == ""
    for g, w in zip(got[1:-1], want[1:-1]):
        g, w = g.split("\t"), w.split("\t")
        assert len(g) == len(w) == 18 and all(g[c] == w[c] for c in range(18) if c not in S_COLS), (g, w)
        for c in S_COLS:  # S to 1e-5 and half a unit of %.4f
            assert abs(float(g[c]) - float(w[c])) <= 6e-5, (c, g, w)


def _verdicts(text):
    """{(a, b, position, base): verdict} of a Paired_Cells.txt"""
    out = {}
    for line in text.split("\n")[1:-1]:
        f = line.split("\t")
        out[(f[0], f[1], int(f[3]) - START, "ACGT".index(f[4][-1]))] = f[VERDICT_COL]
    return out


def test_files_equal_the_model(tmp_path, monkeypatch):
    d = tmp_path
    monkeypatch.delenv("AMPLISOLVE_LIST_DIR_AS", raising=False)
    bases, listed, masked = _write(d)
    env = dict(AMPLISOLVE_REFBASES_FILE=str(d / "r.txt"))
    exp = _model(d, listed, masked)
    print(exp["Paired_Summary.txt"], exp["Paired_Pairs.txt"])
    assert "pairs=10\npositions=200\n" in exp["Paired_Summary.txt"] and "P1_T\tNONE\t0\t0\t0\t0\t0\n" in exp["Paired_Pairs.txt"]
    r = _run(_args(d, "one"), d, **env)
    assert r.returncode == 0, r.stdout[-800:] + r.stderr[-300:]
    assert "10 pairs of 10 files in 1 chunks, 1 batches" in r.stdout, r.stdout[-400:]
    _same(d, "one", exp)
    r = _run(_args(d, "chunks"), d, AMPLISOLVE_CHUNK_BYTES="7000", AMPLISOLVE_THREADS="2", **env)  # two files per chunk: the same files
    assert r.returncode == 0, r.stdout[-800:] + r.stderr[-300:]
    assert "10 pairs of 10 files in 5 chunks" in r.stdout and "1 batches" not in r.stdout, r.stdout[-400:]
    _same(d, "chunks", exp)
    assert (d / "chunks" / "Paired_Cells.txt").read_text() == (d / "one" / "Paired_Cells.txt").read_text()  # a pair's bytes do not depend on its batch
    # the required outcomes, read from the device's own file
    _, _, sites = planted()
    got, want = _verdicts((d / "one" / "Paired_Cells.txt").read_text()), _verdicts(exp["Paired_Cells.txt"])
    for kind in ("somatic_fall", "somatic_gone"):
        for k, p, y in sites[kind]:
            assert got[(f"P{k + 1}_T", f"P{k + 1}_N", p, y)] == "HIGHER_IN_A"
    for kind in ("het", "hom"):
        for k, p, y in sites[kind]:
            for a, b in (("T", "N"), ("F", "T"), ("F", "N")):
                assert got[(f"P{k + 1}_{a}", f"P{k + 1}_{b}", p, y)] == "SHARED"
    for k, p, y in sites["lost"]:
        assert got[(f"P{k + 1}_T", f"P{k + 1}_N", p, y)] == "LOWER_IN_A"
    planted_cells = {(p, y) for lst in sites.values() for _, p, y in lst}
    called = lambda v: sum(1 for (a, b, p, y), x in v.items() if (p, y) not in planted_cells and x in ("HIGHER_IN_A", "LOWER_IN_A"))
    assert called(got) <= 2 * called(want)


def test_exit_status_and_refusals(tmp_path):
    d = tmp_path
    _write(d)
    env = dict(AMPLISOLVE_REFBASES_FILE=str(d / "r.txt"))
    r = _run([f"panel_design={d / 'none.bed'}" if x.startswith("panel_design=") else x for x in _args(d, "o")], d, **env)
    assert r.returncode == 1 and "failed" in r.stdout and not os.path.exists(d / "o")
    r = _run(_args(d, "o"), d, AMPLISOLVE_REFBASES_FILE=str(d / "none.txt"))
    assert r.returncode == 1 and "failed" in r.stdout and not os.path.exists(d / "o")
    (d / "two.txt").write_text("P2_F\tP2_N\nP3_T\tP1_N\n")
    r = _run(_args(d, "o", pairs="two.txt", q_min=5, min_vaf=0, depth_cutoff=0), d, **env)
    assert r.returncode == 0 and sorted(os.listdir(d / "o")) == FILES
    assert (d / "o" / "Paired_Pairs.txt").read_text().count("\n") == 3 and "pairs=2\n" in (d / "o" / "Paired_Summary.txt").read_text()
