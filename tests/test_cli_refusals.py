"""What the project's nine own command lines refuse before they open the device: a wrong number of tokens (the usage text), a bad
value, and AMPLISOLVE_WORLD_SIZE=2.  The exit status is 1, stdout is exactly the text below, stderr is empty and no output directory
appears.  None of these runs reaches the device, so they need no GPU; the refusals that do (a missing directory, a missing reference
file) stay with the tests/test_gpu_*_cli.py files, from whose refusal tables the tokens and the bad values here are taken."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "amplisolve_amd", "bin")
ORDER = "\n\tAll arguments are required, in this order"

# executable -> (its tokens in order with values it accepts, how many tokens the usage case passes, the usage text,
#                [(key, bad value, what the command answers after "<executable> failed: ")])
COMMANDS = {
    "AmpliSolveLeaveOneOut": (
        ["panel_design=p.bed", "reference_genome=x.fa", "germline_dir=N", "C_value=0.002", "coverage_cutoff=100", "calling_cutoff=100", "output_dir=o"], 4,
        "Usage:\n\tAmpliSolveLeaveOneOut panel_design=<bed> reference_genome=<fasta> germline_dir=<dir> C_value=<float>[,<float>...] "
        "coverage_cutoff=<int> calling_cutoff=<int> output_dir=<dir>" + ORDER + ".\n",
        []),
    "AmpliSolveDetectionLimit": (
        ["errorFile=x", "tumour_dir=y", "output_dir=o", "coverage_cutoff=100", "levels=0.01"], 2,
        "Usage:\n\tAmpliSolveDetectionLimit errorFile=<error table> tumour_dir=<dir> output_dir=<dir> coverage_cutoff=<int> "
        "levels=<float>[,<float>...]" + ORDER + ".\n",
        [("levels", "0.01,2", "levels: '2' is not an allele fraction in (0, 1]"),
         ("levels", "", "levels: one to 8 allele fractions are required"),
         ("levels", ",".join(["0.01"] * 9), "levels: one to 8 allele fractions are required")]),
    "AmpliSolveDetectionPower": (
        ["errorFile=x", "tumour_dir=y", "output_dir=o", "coverage_cutoff=100", "levels=0.01", "confidence=0.95"], 2,
        "Usage:\n\tAmpliSolveDetectionPower errorFile=<error table> tumour_dir=<dir> output_dir=<dir> coverage_cutoff=<int> "
        "levels=<float>[,<float>...] confidence=<0.5 .. 0.99>" + ORDER + ".\n",
        [("confidence", "0.4", "confidence: '0.4' is not a probability in [0.5, 0.99]"),
         ("confidence", "0.995", "confidence: '0.995' is not a probability in [0.5, 0.99]"),
         ("confidence", "", "confidence: '' is not a probability in [0.5, 0.99]"),
         ("confidence", "0.9x", "confidence: '0.9x' is not a probability in [0.5, 0.99]"),
         ("levels", "0.01,2", "levels: '2' is not an allele fraction in (0, 1]"),
         ("levels", "", "levels: one to 8 allele fractions are required"),
         ("levels", ",".join(["0.01"] * 9), "levels: one to 8 allele fractions are required")]),
    "AmpliSolvePanelDispersion": (
        ["panel_design=p.bed", "reference_genome=x.fa", "germline_dir=N", "coverage_cutoff=100", "z_cutoff=4", "output_dir=o"], 4,
        "Usage:\n\tAmpliSolvePanelDispersion panel_design=<bed> reference_genome=<fasta> germline_dir=<dir> coverage_cutoff=<int> "
        "z_cutoff=<float> output_dir=<dir>" + ORDER + ".\n",
        [("z_cutoff", "", "z_cutoff must be a number, got ''"),
         ("z_cutoff", "4x", "z_cutoff must be a number, got '4x'"),
         ("z_cutoff", "nan", "z_cutoff must be a number, got 'nan'")]),
    "AmpliSolveSampleConcordance": (
        ["panel_design=p.bed", "germline_dir=N", "tumour_dir=-", "min_depth=100", "min_sites=5", "same_fraction=0.8", "output_dir=o"], 5,
        "Usage:\n\tAmpliSolveSampleConcordance panel_design=<bed> germline_dir=<dir> tumour_dir=<dir or -> min_depth=<int> "
        "min_sites=<int> same_fraction=<float> output_dir=<dir>" + ORDER + ".\n",
        [("same_fraction", "", "same_fraction must be a number in (0, 1], got ''"),
         ("same_fraction", "0.8x", "same_fraction must be a number in (0, 1], got '0.8x'"),
         ("same_fraction", "nan", "same_fraction must be a number in (0, 1], got 'nan'"),
         ("same_fraction", "0", "same_fraction must be a number in (0, 1], got '0'"),
         ("same_fraction", "-0.5", "same_fraction must be a number in (0, 1], got '-0.5'"),
         ("same_fraction", "1.5", "same_fraction must be a number in (0, 1], got '1.5'"),
         ("min_depth", "0", "min_depth must be an integer >= 1, got '0'"),
         ("min_depth", "x", "min_depth must be an integer >= 1, got 'x'"),
         ("min_sites", "0", "min_sites must be an integer >= 1, got '0'"),
         ("min_sites", "2.5", "min_sites must be an integer >= 1, got '2.5'")]),
    "AmpliSolveContamination": (
        ["panel_design=p.bed", "germline_dir=N", "tumour_dir=-", "output_dir=o", "min_depth=100", "min_sites=20", "min_fraction=0.005"], 5,
        "Usage:\n\tAmpliSolveContamination panel_design=<bed> germline_dir=<dir> tumour_dir=<dir or -> output_dir=<dir> "
        "min_depth=<int> min_sites=<int> min_fraction=<float>" + ORDER + " (usual values: min_depth=100 min_sites=20 min_fraction=0.005).\n",
        [("min_fraction", "", "min_fraction must be a number in (0, 1], got ''"),
         ("min_fraction", "0.01x", "min_fraction must be a number in (0, 1], got '0.01x'"),
         ("min_fraction", "nan", "min_fraction must be a number in (0, 1], got 'nan'"),
         ("min_fraction", "0", "min_fraction must be a number in (0, 1], got '0'"),
         ("min_fraction", "-0.5", "min_fraction must be a number in (0, 1], got '-0.5'"),
         ("min_fraction", "1.5", "min_fraction must be a number in (0, 1], got '1.5'"),
         ("min_depth", "0", "min_depth must be an integer >= 1, got '0'"),
         ("min_depth", "x", "min_depth must be an integer >= 1, got 'x'"),
         ("min_sites", "0", "min_sites must be an integer >= 1, got '0'"),
         ("min_sites", "2.5", "min_sites must be an integer >= 1, got '2.5'")]),
    "AmpliSolveAmpliconCoverage": (
        ["panel_design=p.bed", "germline_dir=N", "tumour_dir=-", "output_dir=o", "coverage_cutoff=100", "min_normals=5", "min_amplicons=3", "z_cutoff=3",
         "gain_ratio=1.3", "loss_ratio=0.7", "exclude_chrom=chrX,chrY"], 7,
        "Usage:\n\tAmpliSolveAmpliconCoverage panel_design=<bed> germline_dir=<dir> tumour_dir=<dir or -> output_dir=<dir> "
        "coverage_cutoff=<int> min_normals=<int> min_amplicons=<int> z_cutoff=<float> gain_ratio=<float> loss_ratio=<float> "
        "exclude_chrom=<comma list or ->" + ORDER + " (usual values: coverage_cutoff=100 "
        "min_normals=5 min_amplicons=3 z_cutoff=3 gain_ratio=1.3 loss_ratio=0.7 exclude_chrom=chrX,chrY).\n",
        [("coverage_cutoff", "-1", "coverage_cutoff must be an integer >= 0, got '-1'"),
         ("coverage_cutoff", "x", "coverage_cutoff must be an integer >= 0, got 'x'"),
         ("min_normals", "0", "min_normals must be an integer >= 1, got '0'"),
         ("min_normals", "2.5", "min_normals must be an integer >= 1, got '2.5'"),
         ("min_amplicons", "0", "min_amplicons must be an integer >= 1, got '0'"),
         ("z_cutoff", "-1", "z_cutoff must be a number >= 0, got '-1'"),
         ("z_cutoff", "nan", "z_cutoff must be a number >= 0, got 'nan'"),
         ("z_cutoff", "3x", "z_cutoff must be a number >= 0, got '3x'"),
         ("gain_ratio", "1", "gain_ratio must be a number > 1, got '1'"),
         ("gain_ratio", "inf", "gain_ratio must be a number > 1, got 'inf'"),
         ("loss_ratio", "0", "loss_ratio must be a number in (0, 1), got '0'"),
         ("loss_ratio", "1", "loss_ratio must be a number in (0, 1), got '1'"),
         ("loss_ratio", "", "loss_ratio must be a number in (0, 1), got ''"),
         ("exclude_chrom", "", "exclude_chrom must be a comma list of chromosomes or -, got ''")]),
    "AmpliSolveSubstitutionSpectrum": (
        ["panel_design=p.bed", "reference_genome=unused.fa", "germline_dir=N", "tumour_dir=-", "output_dir=o", "coverage_cutoff=100", "max_alt_pm=30",
         "min_sites=200", "min_normals=5", "excess_ratio=3", "z_cutoff=10", "asym_delta=0.15"], 7,
        "Usage:\n\tAmpliSolveSubstitutionSpectrum panel_design=<bed> reference_genome=<fasta> germline_dir=<dir> tumour_dir=<dir or -> "
        "output_dir=<dir> coverage_cutoff=<int> max_alt_pm=<int> min_sites=<int> min_normals=<int> excess_ratio=<float> z_cutoff=<float> "
        "asym_delta=<float>" + ORDER + " (usual values: coverage_cutoff=100 max_alt_pm=30 min_sites=200 "
        "min_normals=5 excess_ratio=3 z_cutoff=10 asym_delta=0.15).\n",
        [("coverage_cutoff", "-1", "coverage_cutoff must be an integer >= 0, got '-1'"),
         ("coverage_cutoff", "x", "coverage_cutoff must be an integer >= 0, got 'x'"),
         ("max_alt_pm", "-1", "max_alt_pm must be an integer in [0, 1000], got '-1'"),
         ("max_alt_pm", "1001", "max_alt_pm must be an integer in [0, 1000], got '1001'"),
         ("max_alt_pm", "3.5", "max_alt_pm must be an integer in [0, 1000], got '3.5'"),
         ("min_sites", "0", "min_sites must be an integer >= 1, got '0'"),
         ("min_normals", "0", "min_normals must be an integer >= 1, got '0'"),
         ("min_normals", "2.5", "min_normals must be an integer >= 1, got '2.5'"),
         ("excess_ratio", "1", "excess_ratio must be a number > 1, got '1'"),
         ("excess_ratio", "inf", "excess_ratio must be a number > 1, got 'inf'"),
         ("z_cutoff", "-1", "z_cutoff must be a number >= 0, got '-1'"),
         ("z_cutoff", "nan", "z_cutoff must be a number >= 0, got 'nan'"),
         ("z_cutoff", "3x", "z_cutoff must be a number >= 0, got '3x'"),
         ("asym_delta", "-0.1", "asym_delta must be a number in [0, 1], got '-0.1'"),
         ("asym_delta", "1.5", "asym_delta must be a number in [0, 1], got '1.5'"),
         ("asym_delta", "", "asym_delta must be a number in [0, 1], got ''")]),
    "AmpliSolveNormalExceedance": (
        ["panel_design=p.bed", "reference_genome=unused.fa", "germline_dir=N", "tumour_dir=-", "output_dir=o", "coverage_cutoff=100", "calling_cutoff=100",
         "min_alt_reads=3", "min_vaf_pm=0", "min_normals=10", "max_normals=0"], 7,
        "Usage:\n\tAmpliSolveNormalExceedance panel_design=<bed> reference_genome=<fasta> germline_dir=<dir> tumour_dir=<dir or -> "
        "output_dir=<dir> coverage_cutoff=<int> calling_cutoff=<int> min_alt_reads=<int> min_vaf_pm=<int> min_normals=<int> max_normals=<int>"
        + ORDER + " (usual values: coverage_cutoff=100 calling_cutoff=100 min_alt_reads=3 min_vaf_pm=0 min_normals=10 max_normals=0).\n",
        [("coverage_cutoff", "-1", "coverage_cutoff must be an integer >= 0, got '-1'"),
         ("coverage_cutoff", "x", "coverage_cutoff must be an integer >= 0, got 'x'"),
         ("calling_cutoff", "-1", "calling_cutoff must be an integer >= 0, got '-1'"),
         ("calling_cutoff", "1e2", "calling_cutoff must be an integer >= 0, got '1e2'"),
         ("min_alt_reads", "-1", "min_alt_reads must be an integer >= 0, got '-1'"),
         ("min_alt_reads", "2.5", "min_alt_reads must be an integer >= 0, got '2.5'"),
         ("min_vaf_pm", "-1", "min_vaf_pm must be an integer in [0, 1000], got '-1'"),
         ("min_vaf_pm", "1001", "min_vaf_pm must be an integer in [0, 1000], got '1001'"),
         ("min_normals", "-1", "min_normals must be an integer >= 0, got '-1'"),
         ("min_normals", "", "min_normals must be an integer >= 0, got ''"),
         ("max_normals", "-1", "max_normals must be an integer in [0, 65534], got '-1'"),
         ("max_normals", "65535", "max_normals must be an integer in [0, 65534], got '65535'"),
         ("max_normals", "3x", "max_normals must be an integer in [0, 65534], got '3x'")]),
}


def _run(exe, tokens, cwd, **env):
    e = dict(os.environ, **env)
    if "AMPLISOLVE_WORLD_SIZE" not in env:
        e.pop("AMPLISOLVE_WORLD_SIZE", None)
    return subprocess.run([os.path.join(BIN, exe)] + tokens, capture_output=True, text=True, cwd=cwd, env=e, timeout=60)


def _refused(r, stdout, cwd, what):
    assert (r.returncode, r.stdout, r.stderr) == (1, stdout, ""), what
    assert not os.path.exists(cwd / "o"), what  # refused before anything is written


@pytest.mark.parametrize("exe", sorted(COMMANDS))
def test_refused_before_the_device(exe, tmp_path):
    tokens, n_usage, usage, bad_values = COMMANDS[exe]
    _refused(_run(exe, tokens[:n_usage], tmp_path), usage, tmp_path, "usage")
    for key, bad, answer in bad_values:
        t = [f"{key}={bad}" if x.startswith(key + "=") else x for x in tokens]
        assert t != tokens
        _refused(_run(exe, t, tmp_path), f"{exe} failed: {answer}\n", tmp_path, (key, bad))
    _refused(_run(exe, tokens, tmp_path, AMPLISOLVE_WORLD_SIZE="2"),
             f"{exe} failed: {exe} runs on one GPU: AMPLISOLVE_WORLD_SIZE > 1 is not supported\n", tmp_path, "AMPLISOLVE_WORLD_SIZE=2")
