"""The detection limit pinned to the reference's own callVariants (oracle/_ref/AmpliSolveVariantCalling_noFisher).  On fresh panels
every tumour file is written three times with SPIKED counts: at every line whose pair (line, base taken in rotation) has status OK
and whose reference base has the reads to give, that base's counts become (min_fw, min_bw), (min_fw - 1, min_bw) and
(min_fw, min_bw - 1) -- reads moved from the reference base, so FW, BW and the RD column stay as they were.  The reference must call
every spiked pair of the first copy and none of the second and third.  CPU: limits from the model (tests/limit_model.py).  GPU: limits
read from AmpliSolveDetectionLimit's files (run with AMPLISOLVE_LIMIT_VERIFY=all), whose Called column also equals the Summary of
the project's AmpliSolveVariantCalling on the unspiked files and whose summary counts equal the model's."""
import collections
import os
import subprocess

import numpy as np
import pytest

from amplisolve_amd.hostio import HostCohort, read_error_table
from oracle import pyoracle as orc
from tests import limit_model as lm
from tests.test_callvariants_vs_reference import _fresh

pytestmark = pytest.mark.skipif(not (os.path.exists(orc.REF_VC_NOFISHER) and os.path.exists(orc.REF_EE_DRIVER)),
                                reason="oracle/_ref is absent (make -C oracle builds it where the reference's sources are present)")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "amplisolve_amd", "bin")
LEVELS = (0.002, 0.005, 0.02)
ABSENT = np.iinfo(np.int32).min
# (seed, variations of the panel and the tumour files, coverage_cutoff); depth 2000: the reference base always has the reads to give
CASES = [(81, (), 100), (82, ("bed_twice",), 100), (83, ("aseq_own_rd",), 30), (84, ("bed_twice", "aseq_own_rd"), 100)]


def _cohort(d, table):
    co = HostCohort(table, "T", is_error_table=True, keep_line_no=True)
    ref, thr = read_error_table(table)
    return co, ref, thr


def _model_limits(co, ref, thr, cov):
    """per tumour file: {data line index: (chrom, pos, ref, {nt: (status, min_fw, min_bw, called)})} from the model, scanning from k = 1"""
    rdp = co.rd_plane()
    out = {}
    for t, name in enumerate(co.names):
        per = {}
        for r in range(co.P + co.E):
            line = int(co.line_no[t, r])
            if line < 0:
                continue
            p = r if r < co.P else int(co.ext_pos[r - co.P])
            if ref[p] > 3:
                continue
            rec = co.recs[t, r]
            RD = int(rec.astype(np.int64).sum()) if rdp is None or rdp[t, r] == ABSENT else int(rdp[t, r])
            c, x = co.position(p)
            per[line] = (c, int(x), int(ref[p]), {nt: lm.pair_limit(rec, RD, nt, thr[0, nt, p], thr[1, nt, p], cov) for nt in range(4) if nt != ref[p]})
        out[name] = per
    return out


def _tumour_file(d, name):
    return next(f for f in sorted(os.listdir(d / "T")) if f.startswith(name + "."))


def _spike_and_run_reference(d, table, limits, cov):
    """write T1 / T2 / T3, run the reference on each; returns (spiked pairs, OK lines, lines left out)"""
    for k in (1, 2, 3):
        (d / f"T{k}").mkdir()
    want = {1: collections.Counter(), 2: collections.Counter(), 3: collections.Counter()}
    n_ok = n_left = turn = 0
    for name, per in limits.items():
        fname = _tumour_file(d, name)
        lines = (d / "T" / fname).read_text().splitlines()
        copies = {k: list(lines) for k in (1, 2, 3)}
        for li in range(1, len(lines)):
            if li - 1 not in per:
                continue
            c, x, ref, pairs = per[li - 1]
            tok = lines[li].split("\t")
            assert (tok[0], int(tok[1])) == (c, x)
            nt = [b for b in range(4) if b != ref][turn % 3]
            turn += 1
            st, mf, mb, _ = pairs[nt]
            if st != lm.OK:
                continue
            n_ok += 1
            tot, rev = [int(v) for v in tok[6:10]], [int(v) for v in tok[11:15]]
            fw = [a - b for a, b in zip(tot, rev)]
            if fw[ref] + fw[nt] - mf < 0 or rev[ref] + rev[nt] - mb < 0:
                n_left += 1  # the reference base does not have the reads to give
                continue
            for k, (kf, kb) in ((1, (mf, mb)), (2, (mf - 1, mb)), (3, (mf, mb - 1))):
                f2, r2 = list(fw), list(rev)
                f2[ref], f2[nt] = fw[ref] + fw[nt] - kf, kf
                r2[ref], r2[nt] = rev[ref] + rev[nt] - kb, kb
                t2 = list(tok)
                t2[6:10] = [str(a + b) for a, b in zip(f2, r2)]
                t2[11:15] = [str(b) for b in r2]
                assert sum(f2) == sum(fw) and sum(r2) == sum(rev)
                copies[k][li] = "\t".join(t2)
                want[k][(c, str(x), f"{'ACGT'[ref]}->{'ACGT'[nt]}", tok[10], str(sum(fw)), str(sum(rev)), str(kf), str(kb))] += 1
        for k in (1, 2, 3):
            (d / f"T{k}" / fname).write_text("\n".join(copies[k]) + "\n")
    rows = {}
    for k in (1, 2, 3):
        r = subprocess.run([orc.REF_VC_NOFISHER, f"errorFile={table}", f"tumour_dir=T{k}", f"output_dir=rv{k}", f"coverage_cutoff={cov}", "p_value=0.05"],
                           capture_output=True, text=True, cwd=d)
        assert r.returncode == 0, r.stdout[-400:]
        body = [l.split("\t") for l in (d / f"rv{k}" / "Summary_Variant_Info.txt").read_text().splitlines()[1:]]
        # a row is known by position, substitution, RD / RD_fw / RD_bw and the two read counts (multisets: a position may be listed twice)
        rows[k] = collections.Counter(tuple(g[1:7]) + tuple(g[8:10]) for g in body)
    got, exp = rows, want
    missing = exp[1] - got[1]
    assert not missing, list(missing.items())[:5]                       # every spiked pair of the first copy is called
    for k in (2, 3):
        hit = [key for key in exp[k] if got[k][key] > 0]
        assert not hit, (k, hit[:5])                                    # one read less on either strand: not called
    return sum(want[1].values()), n_ok, n_left


@pytest.mark.parametrize("seed,what,cov", CASES)
def test_reference_calls_at_the_models_limit_and_not_one_read_below(tmp_path, monkeypatch, seed, what, cov):
    d = tmp_path
    table = _fresh(d, seed, what, S=6, T=3, depth=2000, amplicons=4)
    monkeypatch.chdir(d)
    co, ref, thr = _cohort(d, table)
    n_spiked, n_ok, n_left = _spike_and_run_reference(d, table, _model_limits(co, ref, thr, cov), cov)
    assert n_spiked > 500 and n_left <= n_ok / 5, (n_spiked, n_ok, n_left)


def _read_limit_file(path):
    rows = [l.split("\t") for l in open(path).read().splitlines()]
    assert rows[0] == ["Chrom", "Position", "Ref", "Alt", "RD", "RD_fw", "RD_bw", "Thr_fw", "Thr_bw", "MinReads_fw", "MinReads_bw", "MinAF", "Status",
                       "Reads_fw", "Reads_bw", "Called"]
    return rows[1:]


@pytest.mark.gpu
@pytest.mark.parametrize("seed,what,cov", CASES)
def test_reference_calls_at_the_command_lines_limit_and_not_one_read_below(tmp_path, monkeypatch, seed, what, cov):
    d = tmp_path
    table = _fresh(d, seed, what, S=6, T=3, depth=2000, amplicons=4)
    monkeypatch.chdir(d)
    env = dict(os.environ, AMPLISOLVE_LIMIT_VERIFY="all")
    r = subprocess.run([os.path.join(BIN, "AmpliSolveDetectionLimit"), f"errorFile={table}", "tumour_dir=T", "output_dir=dl", f"coverage_cutoff={cov}",
                        "levels=" + ",".join(str(v) for v in LEVELS)], capture_output=True, text=True, cwd=d, env=env)
    assert r.returncode == 0, r.stdout[-800:]
    assert " 0 differences" in r.stdout
    co, ref, thr = _cohort(d, table)
    model = _model_limits(co, ref, thr, cov)
    codes = {"OK": lm.OK, "LOWDEPTH": lm.LOWDEPTH, "NOESTIMATE": lm.NOESTIMATE, "UNREACHABLE": lm.UNREACHABLE}
    limits, called = {}, collections.Counter()
    for name, per in model.items():
        rows = _read_limit_file(d / "dl" / f"{name}_detection_limits.txt")
        assert len(rows) == 3 * len(per)
        mine = {}
        for j, line in enumerate(sorted(per)):  # rows in the file's line order, three per line, bases in A, C, G, T order
            c, x, rf, pairs = per[line]
            cell = {}
            for g, nt in zip(rows[3 * j:3 * j + 3], sorted(pairs)):
                assert g[:4] == [c, str(x), "ACGT"[rf], "ACGT"[nt]], (g, c, x)
                st = codes[g[12]]
                mf, mb = (int(g[9]), int(g[10])) if st == lm.OK else (0, 0)
                assert (g[9] == ".") == (st != lm.OK) and (g[11] == ".") == (st != lm.OK)
                cell[nt] = (st, mf, mb, g[15] == "YES")
                assert cell[nt] == pairs[nt], (name, g, pairs[nt])  # the command line's cell is the model's
                if st == lm.OK:
                    assert g[11] == f"{float(lm.min_af(mf, mb, int(g[4]))):.6g}"
                if g[15] == "YES":
                    called[(c, str(x), f"{g[2]}->{g[3]}", g[4], g[5], g[6], g[13], g[14])] += 1
            mine[line] = (c, x, rf, cell)
        limits[name] = mine
    n_spiked, n_ok, n_left = _spike_and_run_reference(d, table, limits, cov)
    assert n_spiked > 500 and n_left <= n_ok / 5, (n_spiked, n_ok, n_left)
    # Called == what the project's own variant calling emits for the unspiked files
    r = subprocess.run([os.path.join(BIN, "AmpliSolveVariantCalling"), f"errorFile={table}", "tumour_dir=T", "output_dir=vc", f"coverage_cutoff={cov}",
                        "p_value=0.05"], capture_output=True, text=True, cwd=d)
    assert r.returncode == 0, r.stdout[-400:]
    body = [l.split("\t") for l in (d / "vc" / "Summary_Variant_Info.txt").read_text().splitlines()[1:]]
    assert collections.Counter(tuple(g[1:7]) + tuple(g[8:10]) for g in body) == called and len(body) > 20
    # the summary: the device's counters, rechecked cells moved, equal the model's
    exp = lm.limit_model(co.recs, co.P, thr, ref, cov, E=co.E, ext_pos=co.ext_pos, rd=co.rd_plane(), levels=LEVELS)
    srows = [l.split("\t") for l in (d / "dl" / "Summary_Detection_Limits.txt").read_text().splitlines()]
    assert srows[0] == ["Filename", "Lines", "NoRefLines", "Pairs", "OK", "LOWDEPTH", "NOESTIMATE", "UNREACHABLE"] + [f"MinAF<={v:g}" for v in LEVELS]
    by_name = {g[0]: [int(v) for v in g[1:]] for g in srows[1:]}
    for t, name in enumerate(co.names):
        c = exp["counts"][t]
        lines = int((co.line_no[t] >= 0).sum())
        assert by_name[name] == [lines, int(c[0]), int(c[1:5].sum()), int(c[1]), int(c[2]), int(c[3]), int(c[4])] + [int(v) for v in c[6:]], name


@pytest.mark.gpu
def test_command_line_refusals(tmp_path):
    exe = os.path.join(BIN, "AmpliSolveDetectionLimit")
    r = subprocess.run([exe, "errorFile=x", "tumour_dir=y"], capture_output=True, text=True)
    assert r.returncode == 1 and "Usage" in r.stdout
    for levels, env in (("0.01,2", {}), ("", {}), (",".join(["0.01"] * 9), {}), ("0.01", {"AMPLISOLVE_WORLD_SIZE": "2"})):
        r = subprocess.run([exe, "errorFile=x", "tumour_dir=y", f"output_dir={tmp_path}/o", "coverage_cutoff=100", f"levels={levels}"],
                           capture_output=True, text=True, env=dict(os.environ, **env))
        assert r.returncode == 1 and "failed" in r.stdout
