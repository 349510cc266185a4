"""What computeIndelCounts refuses before it opens the device: a command line without its required keys or with an unknown one (the
usage text), and input files that cannot be read.  Exit status 1, nothing on stderr, no output file.  None of these runs reaches the
device, so they pass with and without one."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "amplisolve_amd", "bin", "computeIndelCounts")
USAGE = ("Usage:\n\tcomputeIndelCounts vcf=<dummyVCF.txt> bam=<file.bam> [threads=<int>] [mbq=<int>] [mrq=<int>] [mdc=<int>] [refbases=<path>] out=<dir>\n"
         "\tvcf: every position of the panel, one per line (chr pos ...); mbq / mrq / mdc: minimum quality of the base in front of the\n"
         "\tjunction, read (mapping) quality and depth of coverage (20 20 20 recommended); writes <out>/<bam name>.INDEL.PILEUP.ASEQ\n"
         "\t(ref A everywhere: A = reads with neither, C = reads with an insertion, G = reads with a deletion behind the position) and\n"
         "\t<out>/<bam name>.INDEL.LENGTHS.txt (chr pos INS|DEL len count; len 32 means >= 32); refbases: also write the table\n"
         "\t`chrom pos A` to hand to the commands as AMPLISOLVE_REFBASES_FILE.  out must not be the directory of the substitution\n"
         "\tcount files: the commands take every *.ASEQ file of a directory\n")


def _run(tmp_path, *tokens):
    return subprocess.run([EXE, *tokens], cwd=tmp_path, capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("tokens", [(), ("vcf=v.txt", "bam=a.bam"), ("vcf=v.txt", "out=o"), ("bam=a.bam", "out=o"), ("vcf=v.txt", "bam=a.bam", "out=o", "depth=3"),
                                    ("vcf=v.txt", "bam=a.bam", "out=o", "mbq"), ("vcf=", "bam=a.bam", "out=o")])
def test_usage(tmp_path, tokens):
    r = _run(tmp_path, *tokens)
    assert (r.returncode, r.stdout, r.stderr) == (1, USAGE, "")
    assert "out must not be the directory of the substitution" in " ".join(USAGE.split())
    assert os.listdir(tmp_path) == []


def test_unreadable_files(tmp_path):
    (tmp_path / "o").mkdir()
    (tmp_path / "v.txt").write_text("chr1\t100\n")
    r = _run(tmp_path, "vcf=missing.txt", "bam=a.bam", "out=o", "refbases=o/ref.txt")
    assert (r.returncode, r.stdout, r.stderr) == (1, "computeIndelCounts: cannot open missing.txt\n", "")
    r = _run(tmp_path, "vcf=v.txt", "bam=a.bam", "out=o", "refbases=o/ref.txt")
    assert (r.returncode, r.stdout, r.stderr) == (1, "computeIndelCounts: cannot open a.bam\n", "")
    assert os.listdir(tmp_path / "o") == []


def test_the_host_export_refuses_the_same(tmp_path):
    from amplisolve_amd import host_lib

    lib = host_lib()
    assert lib.ampli_host_compute_indel_counts(None, b"a.bam", b"o", None, 2, 20, 20, 20, None) != 0
    rc = lib.ampli_host_compute_indel_counts(str(tmp_path / "v.txt").encode(), str(tmp_path / "a.bam").encode(), str(tmp_path).encode(), None, 2, 20, 20, 20, None)
    assert rc != 0 and b"cannot open" in lib.ampli_host_last_error()
    assert os.listdir(tmp_path) == []
