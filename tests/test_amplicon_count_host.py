"""The host side of computeAmpliconCounts without a device: the builder of the sorted amplicon arrays (ampli_host_amplicon_arrays: BED
rows + the BAM header's reference names -> lo / hi / reach / amp_off and the permutation back to BED order) against the model's, and what
the command line refuses before it opens the device -- the usage text, bad numbers, layers= equal to out=, unreadable inputs.  Exit
status 1, nothing on stderr, no output file.  None of these runs reaches the device, so they pass with and without one."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import amplicon_count_model as am

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "amplisolve_amd", "bin", "computeAmpliconCounts")
REFS = ["chr1", "chr8", "chrX"]


def arrays(tmp_path, bed_text, refs=REFS, cap=64):
    from amplisolve_amd import host_lib

    (tmp_path / "p.bed").write_text(bed_text)
    lo, hi, reach = (np.full(cap, 7, np.uint64) for _ in range(3))
    amp_off, row_of, n_rows = np.full(cap + 1, 7, np.int64), np.full(cap, 7, np.int32), C.c_int64(-1)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    A = host_lib().ampli_host_amplicon_arrays(str(tmp_path / "p.bed").encode(), "\n".join(refs).encode(), cap, ptr(lo), ptr(hi), ptr(reach), ptr(amp_off), ptr(row_of),
                                              C.byref(n_rows))
    return A, lo, hi, reach, amp_off, row_of, n_rows.value


def bed(rows):
    return "".join(f"{c}\t{s}\t{e}\tamp{k}\t.\tGENE{k % 3}\n" for k, (c, s, e) in enumerate(rows))


def test_nested_repeated_and_unknown_rows_against_the_model(tmp_path):
    rows = [("chr8", 500, 640), ("chr1", 1000, 1300), ("chr1", 1100, 1150), ("chr22", 10, 90), ("chr1", 1000, 1300), ("chr1", 1000, 1100), ("chrX", 7, 7),
            ("chr1", 1160, 1180), ("chrUn", 1, 5), ("chr1", 900, 1001)]
    A, lo, hi, reach, amp_off, row_of, n_rows = arrays(tmp_path, bed(rows))
    known = [k for k, r in enumerate(rows) if r[0] in REFS]
    want = am.make_amplicons([(REFS.index(rows[k][0]), rows[k][1], rows[k][2]) for k in known])
    assert (A, n_rows) == (len(known), len(rows)) == (8, 10)
    assert np.array_equal(lo[:A], want.lo) and np.array_equal(hi[:A], want.hi) and np.array_equal(reach[:A], want.reach)
    assert np.array_equal(amp_off[:A + 1], want.amp_off) and row_of[:A].tolist() == [known[i] for i in want.row_of.tolist()]
    assert np.all(lo[A:] == 7) and np.all(amp_off[A + 1:] == 7) and np.all(row_of[A:] == 7)  # nothing behind what the contract names
    # sorted by lo then hi, the repeated row in BED order; reach is monotone though hi is not
    assert row_of[:A].tolist() == [9, 5, 1, 4, 2, 7, 0, 6] and np.all(np.diff(reach[:A].astype(np.int64)) >= 0) and np.any(np.diff(hi[:A].astype(np.int64)) < 0)


def test_empty_malformed_and_too_many(tmp_path):
    assert arrays(tmp_path, "")[::6] == (0, 0)
    A, lo, hi, reach, amp_off, row_of, n_rows = arrays(tmp_path, "chrom\tstart\tend\n\nchr1\t0\t10\nchr1\t20\t10\nchr1\t5\t5\n")
    assert (A, n_rows) == (1, 4) and amp_off[:2].tolist() == [0, 1] and row_of[0] == 3  # a header line, start 0 and end < start stay out
    assert arrays(tmp_path, bed([("chr1", 1, 10)] * 3), cap=2)[0] < 0
    from amplisolve_amd import host_lib

    assert b"more amplicons than the buffers hold" in host_lib().ampli_host_last_error()
    assert arrays(tmp_path, bed([("chr1", 1, 2 ** 31 - 1), ("chr8", 1, 5)]))[0] < 0  # W >= 2^31
    assert arrays(tmp_path, bed([("chr1", 1, 10)]), refs=[])[0] == 0


USAGE_HEAD = ("Usage:\n\tcomputeAmpliconCounts vcf=<dummyVCF.txt> bam=<file.bam> bed=<panel.bed> [threads=<int>] [mbq=<int>] [mrq=<int>] [mdc=<int>]\n"
              "\t                      [min_overlap=<int>] [layers=<dir>] out=<dir>\n")


def _run(tmp_path, *tokens):
    return subprocess.run([EXE, *tokens], cwd=tmp_path, capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("tokens", [(), ("vcf=v.txt", "bam=a.bam", "out=o"), ("vcf=v.txt", "bed=p.bed", "out=o"), ("bam=a.bam", "bed=p.bed", "out=o"),
                                    ("vcf=v.txt", "bam=a.bam", "bed=p.bed"), ("vcf=v.txt", "bam=a.bam", "bed=p.bed", "out=o", "depth=3"),
                                    ("vcf=v.txt", "bam=a.bam", "bed=p.bed", "out=o", "mbq"), ("vcf=v.txt", "bam=a.bam", "bed=", "out=o")])
def test_usage(tmp_path, tokens):
    r = _run(tmp_path, *tokens)
    assert r.returncode == 1 and r.stdout.startswith(USAGE_HEAD) and r.stderr == ""
    assert "layers must differ from out" in " ".join(r.stdout.split()) and os.listdir(tmp_path) == []


def test_bad_numbers_and_unreadable_files(tmp_path):
    (tmp_path / "o").mkdir()
    (tmp_path / "v.txt").write_text("chr1\t100\n")
    (tmp_path / "a.bam").write_bytes(b"not a bam")
    (tmp_path / "p.bed").write_text("chr1\t90\t110\tamp\t.\tG\n")
    ok = ("vcf=v.txt", "bam=a.bam", "bed=p.bed", "out=o")
    for token, what in (("min_overlap=0", "min_overlap must be an integer in [1, 100], got '0'"), ("min_overlap=101", "min_overlap must be an integer in [1, 100], got '101'"),
                        ("min_overlap=5x", "min_overlap must be an integer in [1, 100], got '5x'"), ("mbq=-1", "mbq must be an integer in [0, 255], got '-1'"),
                        ("mdc=", "mdc must be an integer >= 0, got ''"), ("threads=0", "threads must be an integer in [1, 1024], got '0'"),
                        ("layers=o", "layers= must differ from out=: the commands take every *.ASEQ file of a directory")):
        r = _run(tmp_path, *ok, token)
        assert (r.returncode, r.stdout, r.stderr) == (1, f"computeAmpliconCounts: {what}\n", ""), token
    for k, name in enumerate(("missing.txt", "missing.bam", "missing.bed")):
        tokens = list(ok)
        tokens[k] = tokens[k].split("=")[0] + "=" + name
        r = _run(tmp_path, *tokens)
        assert (r.returncode, r.stdout, r.stderr) == (1, f"computeAmpliconCounts: cannot open {name}\n", ""), name
    assert os.listdir(tmp_path / "o") == []


def test_the_host_export_refuses_the_same(tmp_path):
    from amplisolve_amd import host_lib

    lib = host_lib()
    assert lib.ampli_host_compute_amplicon_counts(None, b"a.bam", b"p.bed", b"o", None, 2, 20, 20, 20, 50, None) != 0
    args = [str(tmp_path / n).encode() for n in ("v.txt", "a.bam", "p.bed")] + [str(tmp_path).encode(), None]
    assert lib.ampli_host_compute_amplicon_counts(*args, 2, 20, 20, 20, 0, None) != 0 and b"min_overlap must be" in lib.ampli_host_last_error()
    assert lib.ampli_host_compute_amplicon_counts(*args, 2, 20, 20, 20, 50, None) != 0 and b"cannot open" in lib.ampli_host_last_error()
    assert os.listdir(tmp_path) == []
