#!/usr/bin/env python3
"""Two builds of the host side (this tree's amplisolve_amd/bin + lib, and another directory's) on the same inputs, on one GPU:
  --bytes  all four executables on the fixtures and on fresh panels; exit status, stdout, stderr and every output file of the two builds
           must be the same bytes outside the ##fileDate= line, TIMING* lines and the <seed>_ prefix of the by-product files' names
           (rand() seeded with time(): EE:581-584), which the executables also print;
  --speed  tools/cli_phases.py's runs (EE + VC on BASELINE configs), the two builds alternating on ONE set of files; per executable
           and config the other build's spread (max - min of its wall_s) is the tolerance for |median(this) - median(other)|.
usage: python tools/compare_host_builds.py --other DIR [--bytes] [--speed] [--reps 5] [--configs c2,c3]     (DIR holds bin/ and lib/)"""
import argparse
import json
import os
import pathlib
import re
import shutil
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from tests.helpers import GOLDEN as G  # noqa: E402
from tests.helpers import write_fresh_panel, write_fresh_tumours  # noqa: E402
from tools.cli_phases import phases  # noqa: E402

SEED = re.compile(r"(_interm_files/)\d+_")


def clean(text):
    return "\n".join(SEED.sub(r"\1SEED_", ln) for ln in text.splitlines() if not ln.startswith(("TIMING", "##fileDate=")))


def tree(out):
    """relative name (seed prefix of the by-product files cut away) -> bytes that must agree"""
    got = {}
    for f in sorted(pathlib.Path(out).rglob("*")):
        if f.is_file():
            rel = str(f.relative_to(out))
            got[re.sub(r"(_interm_files/)\d+_", r"\1SEED_", rel)] = clean(f.read_text(errors="replace"))
    return got


def overflow_panel(d):
    """tests/test_gpu_cli.py::test_variant_calling_cli_recovers_from_queue_and_call_list_overflow: 73 728 calls in one chunk"""
    (d / "T").mkdir()
    head = "chrom\tposition\treference\tduplicate\tThres_A\tThres_C\tThres_G\tThres_T\tGerm_Max_A\tGerm_Max_C\tGerm_Max_G\tGerm_Max_T\n"
    (d / "psn.txt").write_text(head + "".join(f"chr5\t{1000 + i}\tA\tNO\t-2_-2" + "\t0.002000_0.002000" * 3 + "\t-" * 4 + "\n" for i in range(2048)))
    body = "chr\tpos\tdbsnp\tMAF\tref\talt\tA\tC\tG\tT\tRD\tArs\tCrs\tGrs\tTrs\n" + "".join(
        f"chr5\t{1000 + i}\t.\t.\t.\t.\t1880\t40\t40\t40\t2000\t940\t20\t20\t20\n" for i in range(2048))
    for t in range(12):
        (d / "T" / f"K{t:02d}.PILEUP.ASEQ").write_text(body)


def compare_bytes(builds):
    work = pathlib.Path(tempfile.mkdtemp(prefix="ampli_builds_"))
    fresh, over = work / "fresh", work / "over"
    fresh.mkdir(), over.mkdir()
    write_fresh_panel(fresh, 5150, depth=2000, S=9, amplicons=6)
    write_fresh_tumours(fresh, 5150, T=4, depth=2000)
    overflow_panel(over)
    ee = lambda d, C, cov, **env: (["AmpliSolveErrorEstimation", f"panel_design={d}/panel.bed", "reference_genome=x.fa", f"germline_dir={d}/NORMAL", f"C_value={C}",
                                    f"coverage_cutoff={cov}", "default_error=0.01", "output_dir=o"], dict(env, AMPLISOLVE_REFBASES_FILE=f"{d}/refbases.txt"))
    toy, table = f"{G}/toy_subset", f"{G}/toy_subset/expected_positionSpecificNoise_0.0020.txt"
    vc = lambda **env: (["AmpliSolveVariantCalling", f"errorFile={table}", f"tumour_dir={toy}/TUMOUR", "output_dir=o", "coverage_cutoff=100", "p_value=0.05"], env)
    cases = [("toy_subset EE", *ee(toy, "0.002", "100")), ("toy_subset VC", *vc()), ("toy_subset VC one sample per chunk", *vc(AMPLISOLVE_CHUNK_BYTES="1"))]
    cases += [(f"mini_edge EE C={C} cov={cov}", *ee(f"{G}/mini_edge", C, cov)) for C, cov in (("0.002", "100"), ("0.0005", "1"), ("0.05", "1000"))]
    cases += [("irregular EE", *ee(f"{G}/irregular", "0.002", "100")),
              ("overflow panel VC", ["AmpliSolveVariantCalling", f"errorFile={over}/psn.txt", f"tumour_dir={over}/T", "output_dir=o", "coverage_cutoff=100", "p_value=0.05"], {}),
              ("fresh panel EE", ["AmpliSolveErrorEstimation", f"panel_design={fresh}/p.bed", "reference_genome=x.fa", f"germline_dir={fresh}/N", "C_value=0.002",
                                  "coverage_cutoff=100", "default_error=0.01", "output_dir=o"], {"AMPLISOLVE_REFBASES_FILE": f"{fresh}/r.txt"}),
              ("fresh panel LeaveOneOut", ["AmpliSolveLeaveOneOut", f"panel_design={fresh}/p.bed", "reference_genome=x.fa", f"germline_dir={fresh}/N", "C_value=0.002,0.01",
                                           "coverage_cutoff=100", "calling_cutoff=100", "output_dir=o"], {"AMPLISOLVE_REFBASES_FILE": f"{fresh}/r.txt"}),
              ("fresh panel DetectionLimit", ["AmpliSolveDetectionLimit", f"errorFile={fresh}/psn.txt", f"tumour_dir={fresh}/T", "output_dir=o",
                                              "coverage_cutoff=100", "levels=0.01,0.05"], {"AMPLISOLVE_LIMIT_VERIFY": "all"})]
    bad = 0
    for k, (name, cmd, env) in enumerate(cases):
        got = []
        for b, bindir in builds:
            cwd = work / f"case{k}_{b}"
            cwd.mkdir()
            r = subprocess.run([os.path.join(bindir, cmd[0])] + cmd[1:], capture_output=True, text=True, cwd=cwd, timeout=300,
                               env=dict(os.environ, AMPLISOLVE_STRICT_EXIT="1", AMPLISOLVE_TIMING="1", **env))
            got.append((r.returncode, clean(r.stdout), clean(r.stderr), tree(cwd / "o")))
            if name == "fresh panel EE" and b == "this":  # the table the detection limits of BOTH builds read
                shutil.copy(cwd / "o" / "positionSpecificNoise_0.0020.txt", fresh / "psn.txt")
        same = got[0] == got[1]
        bad += 0 if same else 1
        print(f"{name}: exit {got[0][0]} / {got[1][0]}, {len(got[0][3])} files, {sum(len(v) for v in got[0][3].values())} bytes, "
              f"{len(got[0][1])} bytes of stdout: {'IDENTICAL' if same else 'DIFFERENT'}", flush=True)
        if not same:
            for what, x, y in zip(("exit", "stdout", "stderr", "files"), got[0], got[1]):
                if x != y:
                    print(f"   differs: {what}" + (f" {sorted(n for n in set(x) | set(y) if x.get(n) != y.get(n))}" if what == "files" else ""))
    shutil.rmtree(work, ignore_errors=True)
    return bad


def compare_speed(builds, reps, configs):
    walls, names, own = {}, {}, {}  # own: the time in main() outside the wait for the HIP runtime's start-up, whose length is the machine's
    for name in configs:
        cfg = bench.CONFIGS[name]
        d = tempfile.mkdtemp(prefix=f"ampli_builds_{name}_")
        try:
            bench.write_workload_files(d, cfg["P"], cfg["S"], cfg["T"], cfg["depth"])
            env = {"AMPLISOLVE_TIMING": "1", "AMPLISOLVE_STRICT_EXIT": "1", "AMPLISOLVE_REFBASES_FILE": "refbases.txt"}
            for rep in range(reps):
                for b, bindir in builds:
                    for exe, cmd in (("EE", ["AmpliSolveErrorEstimation", "panel_design=panel.bed", "reference_genome=unused.fa", "germline_dir=N", "C_value=0.002",
                                             "coverage_cutoff=100", "default_error=0.01", "output_dir=ee"]),
                                     ("VC", ["AmpliSolveVariantCalling", "errorFile=ee/positionSpecificNoise_0.0020.txt", "tumour_dir=T", "output_dir=vc",
                                             "coverage_cutoff=100", "p_value=0.05"])):
                        rc, wall, _, out, err, rss = bench._run_timed([os.path.join(bindir, cmd[0])] + cmd[1:], d, env)
                        assert rc == 0, out + err
                        ph = phases(err)
                        print(json.dumps({"build": b, "config": name, "exe": exe, "rep": rep, "wall_s": round(wall, 4), "phases": ph}), flush=True)
                        walls.setdefault((name, exe, b), []).append(wall)
                        own.setdefault((name, exe, b), []).append(ph["wall_in_main"] - ph["wait_for_context"])
                        names.setdefault((name, exe, b), set()).update(ph)
        finally:
            shutil.rmtree(d, ignore_errors=True)
    bad = 0
    (other, _), (this, _) = builds  # the other build first in every repetition
    for name in configs:
        for exe in ("EE", "VC"):
            o, t = walls[name, exe, other], walls[name, exe, this]
            spread, diff = max(o) - min(o), statistics.median(t) - statistics.median(o)
            ok = abs(diff) <= spread and names[name, exe, this] == names[name, exe, other]
            bad += 0 if ok else 1
            print(f"SPEED {name} {exe}: {other} median {statistics.median(o):.4f} s (min {min(o):.4f}, max {max(o):.4f}, spread {spread:.4f}); {this} median "
                  f"{statistics.median(t):.4f} s (min {min(t):.4f}, max {max(t):.4f}); difference {diff:+.4f} s: {'WITHIN' if abs(diff) <= spread else 'OUTSIDE'} the spread; "
                  f"TIMING2 phase names {'unchanged' if names[name, exe, this] == names[name, exe, other] else 'CHANGED'}; median wall_in_main - "
                  f"wait_for_context: {other} {statistics.median(own[name, exe, other]):.4f} s, {this} {statistics.median(own[name, exe, this]):.4f} s", flush=True)
    return bad


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--other", required=True, help="directory with the other build's bin/ and lib/")
    ap.add_argument("--bytes", action="store_true")
    ap.add_argument("--speed", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--configs", default="c2,c3")
    a = ap.parse_args()
    builds = [("this", bench.BIN), ("other", os.path.join(os.path.abspath(a.other), "bin"))]
    bad = (compare_bytes(builds) if a.bytes else 0) + (compare_speed(builds[::-1], a.reps, a.configs.split(",")) if a.speed else 0)
    sys.exit(1 if bad else 0)
