"""What computeReadEvidence refuses before it opens the device: a command line without its required keys or with an unknown one (the
usage text), bad numbers, and input files that cannot be read.  Exit status 1, nothing on stderr, no output file.  None of these runs
reaches the device, so they pass with and without one."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "amplisolve_amd", "bin", "computeReadEvidence")
USAGE = ("Usage:\n\tcomputeReadEvidence vcf=<calls.txt> bam=<file.bam> [threads=<int>] [mbq=<int>] [mrq=<int>] [min_alt=<int>] [z_min=<decimal>] out=<dir>\n"
         "\tvcf: the calls to examine, one per line (chr pos id ref alt); ref and alt select the two alleles, an alt of . takes the\n"
         "\tnon-reference base with the most reads, a multi-base or non-ACGT ref or alt leaves the line UNTESTED.  List calls, not the\n"
         "\tpanel: every listed position keeps 3 KB of bins, a sparse list is counted in on-chip memory, and a list of every panel\n"
         "\tposition takes the slow path of one memory update per base and metric (measured: twelve times the time of computeCounts).\n"
         "\tmbq / mrq: minimum base quality and read (mapping) quality, as computeCounts (20 20); min_alt: the reads either allele\n"
         "\tneeds for a verdict (an integer >= 1, default 4); z_min: the score from which a metric is flagged (a decimal > 0, default 3).\n"
         "\tWrites <out>/<bam name>.EVIDENCE.txt (chr pos ref alt n_ref n_alt, then med_ref med_alt z for base quality, MAPQ / 4 and\n"
         "\tdistance to the read's nearer end, then UNTESTED, PASS or a comma-joined subset of LOW_BQ LOW_MQ READ_END; z < 0: the alt\n"
         "\treads rank below the ref reads) and <out>/<bam name>.EVIDENCE.HIST.txt (chr pos nt metric bin count per non-zero bin)\n")


def _run(tmp_path, *tokens):
    return subprocess.run([EXE, *tokens], cwd=tmp_path, capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("tokens", [(), ("vcf=v.txt", "bam=a.bam"), ("vcf=v.txt", "out=o"), ("bam=a.bam", "out=o"), ("vcf=v.txt", "bam=a.bam", "out=o", "mdc=3"),
                                    ("vcf=v.txt", "bam=a.bam", "out=o", "z_min"), ("vcf=", "bam=a.bam", "out=o")])
def test_usage(tmp_path, tokens):
    r = _run(tmp_path, *tokens)
    assert (r.returncode, r.stdout, r.stderr) == (1, USAGE, "")
    assert "List calls, not the panel" in " ".join(USAGE.split()) and "slow path" in USAGE
    assert os.listdir(tmp_path) == []


@pytest.mark.parametrize("token, what", [("threads=0", "threads"), ("threads=x", "threads"), ("mbq=256", "mbq"), ("mbq=-1", "mbq"), ("mrq=2.5", "mrq"), ("mrq=", "mrq"),
                                         ("min_alt=0", "min_alt"), ("min_alt=-3", "min_alt"), ("min_alt=four", "min_alt"), ("z_min=0", "z_min"), ("z_min=-3", "z_min"),
                                         ("z_min=nan", "z_min"), ("z_min=inf", "z_min"), ("z_min=3x", "z_min")])
def test_bad_numbers_are_refused_before_the_files_are_looked_at(tmp_path, token, what):
    (tmp_path / "o").mkdir()
    r = _run(tmp_path, "vcf=missing.txt", "bam=a.bam", "out=o", token)
    assert r.returncode == 1 and r.stderr == "" and r.stdout.startswith("computeReadEvidence: ") and what in r.stdout and "cannot open" not in r.stdout, r.stdout
    assert os.listdir(tmp_path / "o") == []


def test_unreadable_files(tmp_path):
    (tmp_path / "o").mkdir()
    (tmp_path / "v.txt").write_text("chr1\t100\t.\tA\tC\n")
    r = _run(tmp_path, "vcf=missing.txt", "bam=a.bam", "out=o")
    assert (r.returncode, r.stdout, r.stderr) == (1, "computeReadEvidence: cannot open missing.txt\n", "")
    r = _run(tmp_path, "vcf=v.txt", "bam=a.bam", "out=o", "min_alt=1", "z_min=0.5")
    assert (r.returncode, r.stdout, r.stderr) == (1, "computeReadEvidence: cannot open a.bam\n", "")
    assert os.listdir(tmp_path / "o") == []


def test_the_host_export_refuses_the_same(tmp_path):
    from amplisolve_amd import host_lib

    lib = host_lib()
    assert lib.ampli_host_compute_read_evidence(None, b"a.bam", b"o", 2, 20, 20, 4, 3.0, None) != 0
    args = (str(tmp_path / "v.txt").encode(), str(tmp_path / "a.bam").encode(), str(tmp_path).encode())
    assert lib.ampli_host_compute_read_evidence(*args, 2, 20, 20, 4, 3.0, None) != 0 and b"cannot open" in lib.ampli_host_last_error()
    assert lib.ampli_host_compute_read_evidence(*args, 2, 20, 20, 0, 3.0, None) != 0 and b"min_alt" in lib.ampli_host_last_error()
    assert lib.ampli_host_compute_read_evidence(*args, 2, 20, 20, 4, 0.0, None) != 0 and b"z_min" in lib.ampli_host_last_error()
    assert os.listdir(tmp_path) == []
