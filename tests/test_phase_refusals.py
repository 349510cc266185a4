"""What computePhasing refuses before it opens the device: a command line without its required keys or with an unknown one (the usage
text), bad numbers, and input files that cannot be read.  Exit status 1, nothing on stderr, no output file.  None of these runs reaches the
device, so they pass with and without one."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "amplisolve_amd", "bin", "computePhasing")
USAGE = ("Usage:\n\tcomputePhasing vcf=<calls.txt> bam=<file.bam> [threads=<int>] [mbq=<int>] [mrq=<int>] [min_alt=<int>] [min_share=<int>] [q_min=<decimal>]\n"
         "\t               [max_dist=<int>] out=<dir>\n"
         "\tvcf: the calls to pair, one per line (chr pos id ref alt).  Every two lines on one chromosome at most max_dist apart (an integer\n"
         "\t>= 1, default 200) are a pair; lines at the same position are none.  Alignment records are counted, not fragments: overlapping\n"
         "\tmates count twice, as in computeCounts.  Only the next 8 listed positions are partners: a pair further apart in the list is\n"
         "\twritten as NOT_FORMED.  Strands are pooled.  An insertion has no position of its own; a multi-base or non-ACGT ref or alt\n"
         "\tleaves the pair UNTESTED.  List calls, not the panel: a list of every panel position takes\n"
         "\tthe slow path of one memory update per read and pair (measured: 1.2 times computeReadEvidence on such a list).\n"
         "\tmbq / mrq: minimum base quality and read (mapping) quality, as computeCounts (20 20).  A group of reads (alt at both, alt at A\n"
         "\tonly, alt at B only) is present with min_alt reads (an integer >= 1, default 4) that are min_share per cent (0 .. 100, default\n"
         "\t10) of the reads with an alt at either.  Verdicts: CIS (only alt at both), NESTED_B / NESTED_A (B's / A's alt reads are a subset\n"
         "\tof the other's), each with the exact test's score >= q_min (a decimal > 0, default 13), else UNRESOLVED; TRANS (never alt at\n"
         "\tboth), MIXED (all three groups), UNTESTED (a variant without reads among the joint ones).  TRANS and MIXED carry no score\n"
         "\tgate: at low allele fractions the absence of reads with both alts is not significant as an association; exp_aa beside it\n"
         "\tsays how many were expected.\n"
         "\tWrites <out>/<bam name>.PHASE.txt (chr posA refA altA posB refB altB n_joint n_rr n_ra n_ar n_aa n_other exp_aa score verdict;\n"
         "\tthe first letter is the allele at A; score > 0: linked in cis) and <out>/<bam name>.PHASE.MNV.txt (chr pos ref_string\n"
         "\talt_string reads per chain of 2 or 3 consecutive positions that are CIS in pairs)\n")


def _run(tmp_path, *tokens):
    return subprocess.run([EXE, *tokens], cwd=tmp_path, capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("tokens", [(), ("vcf=v.txt", "bam=a.bam"), ("vcf=v.txt", "out=o"), ("bam=a.bam", "out=o"), ("vcf=v.txt", "bam=a.bam", "out=o", "mdc=3"),
                                    ("vcf=v.txt", "bam=a.bam", "out=o", "z_min=3"), ("vcf=v.txt", "bam=a.bam", "out=o", "q_min"), ("vcf=", "bam=a.bam", "out=o")])
def test_usage(tmp_path, tokens):
    r = _run(tmp_path, *tokens)
    assert (r.returncode, r.stdout, r.stderr) == (1, USAGE, "")
    flat = " ".join(USAGE.split())
    for limit in ("counted, not fragments", "Only the next 8 listed positions are partners", "Strands are pooled", "An insertion has no position of its own",
                  "TRANS and MIXED carry no score gate", "List calls, not the panel"):
        assert limit in flat, limit
    assert os.listdir(tmp_path) == []


@pytest.mark.parametrize("token, what", [("threads=0", "threads"), ("threads=x", "threads"), ("mbq=256", "mbq"), ("mbq=-1", "mbq"), ("mrq=2.5", "mrq"), ("mrq=", "mrq"),
                                         ("min_alt=0", "min_alt"), ("min_alt=-3", "min_alt"), ("min_alt=four", "min_alt"), ("min_share=-1", "min_share"),
                                         ("min_share=101", "min_share"), ("min_share=10.5", "min_share"), ("q_min=0", "q_min"), ("q_min=-13", "q_min"), ("q_min=nan", "q_min"),
                                         ("q_min=inf", "q_min"), ("q_min=13x", "q_min"), ("max_dist=0", "max_dist"), ("max_dist=-5", "max_dist"), ("max_dist=1e3", "max_dist")])
def test_bad_numbers_are_refused_before_the_files_are_looked_at(tmp_path, token, what):
    (tmp_path / "o").mkdir()
    r = _run(tmp_path, "vcf=missing.txt", "bam=a.bam", "out=o", token)
    assert r.returncode == 1 and r.stderr == "" and r.stdout.startswith("computePhasing: ") and what in r.stdout and "cannot open" not in r.stdout, r.stdout
    assert os.listdir(tmp_path / "o") == []


def test_unreadable_files(tmp_path):
    (tmp_path / "o").mkdir()
    (tmp_path / "v.txt").write_text("chr1\t100\t.\tA\tC\nchr1\t101\t.\tA\tC\n")
    r = _run(tmp_path, "vcf=missing.txt", "bam=a.bam", "out=o")
    assert (r.returncode, r.stdout, r.stderr) == (1, "computePhasing: cannot open missing.txt\n", "")
    r = _run(tmp_path, "vcf=v.txt", "bam=a.bam", "out=o", "min_alt=1", "min_share=0", "q_min=0.5", "max_dist=1")
    assert (r.returncode, r.stdout, r.stderr) == (1, "computePhasing: cannot open a.bam\n", "")
    assert os.listdir(tmp_path / "o") == []


def test_the_host_export_refuses_the_same(tmp_path):
    from amplisolve_amd import host_lib

    lib = host_lib()
    call = lib.ampli_host_compute_phasing
    assert call(None, b"a.bam", b"o", 2, 20, 20, 4, 10, 13.0, 200, None) != 0
    args = (str(tmp_path / "v.txt").encode(), str(tmp_path / "a.bam").encode(), str(tmp_path).encode())
    assert call(*args, 2, 20, 20, 4, 10, 13.0, 200, None) != 0 and b"cannot open" in lib.ampli_host_last_error()
    for numbers, what in (((0, 20, 20, 4, 10, 13.0, 200), b"threads"), ((2, 256, 20, 4, 10, 13.0, 200), b"mbq"), ((2, 20, -1, 4, 10, 13.0, 200), b"mrq"),
                          ((2, 20, 20, 0, 10, 13.0, 200), b"min_alt"), ((2, 20, 20, 4, 101, 13.0, 200), b"min_share"), ((2, 20, 20, 4, -1, 13.0, 200), b"min_share"),
                          ((2, 20, 20, 4, 10, 0.0, 200), b"q_min"), ((2, 20, 20, 4, 10, float("nan"), 200), b"q_min"), ((2, 20, 20, 4, 10, 13.0, 0), b"max_dist")):
        assert call(*args, *numbers, None) != 0 and what in lib.ampli_host_last_error(), numbers
    assert os.listdir(tmp_path) == []
