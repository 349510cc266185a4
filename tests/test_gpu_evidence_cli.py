"""computeReadEvidence on the GPU (BAM + a list of calls -> .EVIDENCE.txt + .EVIDENCE.HIST.txt; ampli_pileup_evidence over computeCounts'
batch loop, then ampli_evidence_score over the listed lines) against the model of tests/evidence_model.py on the same synthetic BAM files,
byte for byte: a position listed twice, an unknown chromosome, alt given and `.`, unusable alleles; an empty, a corrupt and a truncated
file; and one amplicon with four planted calls whose verdicts the model gives before the device is touched."""
import os
import subprocess

import numpy as np
import pytest

from tests import evidence_model as em
from tests import helpers
from tests.pileup_model import read

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "amplisolve_amd", "bin")
REFS = [("chr1", 100000), ("chr8", 50000), ("chrX", 30000), ("chrUn", 5000)]
AMPS = [(0, 1000, 1120), (0, 1100, 1230), (1, 5000, 5100), (2, 200, 330), (2, 29950, 29999)]


def calls(rng, n=60):
    """the list: n calls inside the amplicons with ref and alt drawn (alt `.` for a third), then a position listed twice with other alleles, a
    chromosome the BAM does not know, an uncovered position and lines whose alleles cannot be used"""
    names = [n_ for n_, _ in REFS]
    lines = []
    for _ in range(n):
        r, s, e = AMPS[int(rng.integers(len(AMPS)))]
        ref = "ACGT"[int(rng.integers(4))]
        alt = "." if rng.random() < 0.34 else "ACGT"[("ACGT".index(ref) + 1 + int(rng.integers(3))) % 4]
        lines.append((names[r], int(rng.integers(s, e + 1)), ref, alt))
    first = lines[0]
    lines += [(first[0], first[1], "ACGT"[("ACGT".index(first[2]) + 1) % 4], "."), first]
    lines += [("chr22", 12, "A", "C"), ("chr8", 40000, "G", "."), ("chr1", 1050, "AT", "A"), ("chr1", 1051, "A", "AT"), ("chr1", 1052, "N", "."), ("chr1", 1053, "c", "c"),
              ("chr1", 1054, "a", "g"), ("chr1", 1055, ".", ".")]
    return lines


def write_vcf(path, lines):
    with open(path, "w") as f:
        f.write("#chr\tpos\tid\tref\talt\n")
        for c, p, ref, alt in lines:
            f.write(f"{c}\t{p}\t.\t{ref}\t{alt}\n")


def model_files(reads, lines, mbq, mrq, min_alt, z_min):
    """(EVIDENCE text, HIST text, Result) the command must write for `reads` on the listed lines"""
    names = [n for n, _ in REFS]
    keys = em.make_keys([(names.index(c), p) for c, p, _, _ in lines if c in names])
    res = em.count(reads, keys, mbq, mrq) if reads else em.Result(np.zeros((len(keys), 4, em.METRICS, em.BINS), np.int64), (0, 0))
    index = {int(k): i for i, k in enumerate(keys.tolist())}
    planes = np.zeros((len(lines), 4, em.METRICS, em.BINS), np.int64)
    for l, (c, p, _, _) in enumerate(lines):
        if c in names:
            planes[l] = res.hist[index[(names.index(c) << 32) | p]]
    return em.files(lines, planes, min_alt, z_min) + (res,)


def run_re(*args, env=None, **kw):
    return subprocess.run([f"{BIN}/computeReadEvidence", *[str(a) for a in args]], capture_output=True, text=True, timeout=300,
                          env=dict(os.environ, AMPLISOLVE_STRICT_EXIT="1", **(env or {})), **kw)


@pytest.mark.parametrize("seed,n_reads,mbq,mrq,min_alt,z_min", [(1, 3000, 20, 20, 4, "3"), (2, 1500, 0, 0, 1, "0.5"), (3, 2500, 21, 5, 10, "2.25")])
def test_the_files_equal_the_model_byte_for_byte(tmp_path, seed, n_reads, mbq, mrq, min_alt, z_min):
    rng = np.random.default_rng(seed)
    reads = em.sharpen(rng, helpers.random_amplicon_reads(rng, REFS, AMPS, n_reads, odd_ops=0.3))
    helpers.write_bam(tmp_path / "S1.bam", REFS, reads, rng=rng, max_block=20000)
    lines = calls(rng)
    write_vcf(tmp_path / "v.txt", lines)
    out = tmp_path / "out"
    out.mkdir()
    ev, hist, res = model_files(reads, lines, mbq, mrq, min_alt, float(z_min))  # before the device is touched
    verdicts = [l.split("\t")[-1] for l in ev.splitlines()]
    assert verdicts.count("UNTESTED") >= 7 and len(set(verdicts)) >= 2 and len(hist.splitlines()) > 200
    r = run_re(f"vcf={tmp_path}/v.txt", f"bam={tmp_path}/S1.bam", "threads=3", f"mbq={mbq}", f"mrq={mrq}", f"min_alt={min_alt}", f"z_min={z_min}", f"out={out}",
               env={"AMPLISOLVE_BAM_BATCH_BYTES": "70000"})  # many small batches: records and even the header span batch boundaries
    assert r.returncode == 0, r.stdout + r.stderr
    assert (out / "S1.EVIDENCE.txt").read_text() == ev
    assert (out / "S1.EVIDENCE.HIST.txt").read_text() == hist
    assert sorted(os.listdir(out)) == ["S1.EVIDENCE.HIST.txt", "S1.EVIDENCE.txt"]  # no temporary file stays
    assert f"{len(reads)} alignment records (0 malformed), {res.stats[0]} kept (mrq {mrq}), {res.stats[1]} columns counted (mbq {mbq}) over {len(lines)} listed lines" in r.stdout
    got = ev.splitlines()
    n = len(lines)
    assert got[n - 9].split("\t")[:2] == got[0].split("\t")[:2] and got[n - 9] == got[0]           # a position listed twice is written twice
    assert got[n - 10].split("\t")[:2] == got[0].split("\t")[:2] and got[n - 10] != got[0]         # ... with the alleles of its own line
    assert got[n - 8].split("\t") == ["chr22", "12", "A", "C", "0", "0"] + ["-1", "-1", "."] * 3 + ["UNTESTED"]  # an unknown chromosome
    assert all(g.endswith("\tUNTESTED") for g in got[n - 6:n - 2] + got[n - 1:])                  # unusable alleles


def test_an_empty_a_corrupt_and_a_truncated_file(tmp_path):
    rng = np.random.default_rng(29)
    lines = calls(rng, 20)
    write_vcf(tmp_path / "v.txt", lines)
    helpers.write_bam(tmp_path / "E.bam", REFS, [])
    (tmp_path / "e").mkdir()
    r = run_re(f"vcf={tmp_path}/v.txt", f"bam={tmp_path}/E.bam", f"out={tmp_path}/e")
    assert r.returncode == 0, r.stdout + r.stderr
    ev, hist, _ = model_files([], lines, 20, 20, 4, 3.0)
    assert (tmp_path / "e" / "E.EVIDENCE.txt").read_text() == ev and len(ev.splitlines()) == len(lines) and all(l.endswith("\tUNTESTED") for l in ev.splitlines())
    assert (tmp_path / "e" / "E.EVIDENCE.HIST.txt").read_text() == hist == ""
    assert sorted(os.listdir(tmp_path / "e")) == ["E.EVIDENCE.HIST.txt", "E.EVIDENCE.txt"]
    reads = helpers.random_amplicon_reads(rng, REFS, AMPS, 800)
    helpers.write_bam(tmp_path / "C.bam", REFS, reads, rng=rng, max_block=5000, corrupt_block_size=(400, 0x7FFFFFFF))
    (tmp_path / "o").mkdir()
    r = run_re(f"vcf={tmp_path}/v.txt", f"bam={tmp_path}/C.bam", f"out={tmp_path}/o")
    assert r.returncode != 0 and "computeReadEvidence: " in r.stdout and "corrupt BAM record at uncompressed byte" in r.stdout
    assert os.listdir(tmp_path / "o") == []
    helpers.write_bam(tmp_path / "T.bam", REFS, reads[:50])  # a file cut off inside a record
    raw = (tmp_path / "T.bam").read_bytes()
    (tmp_path / "T.bam").write_bytes(raw[:len(raw) // 2])
    r = run_re(f"vcf={tmp_path}/v.txt", f"bam={tmp_path}/T.bam", f"out={tmp_path}/o")
    assert r.returncode != 0 and os.listdir(tmp_path / "o") == []


# ---------------------------------------------------------------------------------------------------------------------------
# end to end: one amplicon, 400 reads of 100 bases whose starts are spread over 21 positions, reference base A everywhere, Q40, MAPQ 60.
# Four planted positions with 40 alt (C) reads each:
#   CLEAN    the alt reads have the qualities, the MAPQ and the offsets of the reference reads
#   LOW_BQ   the alt bases are Q20-21 among Q40 reference bases
#   READ_END the alt reads start on the position or at most two bases in front of it (i <= 2); the reference reads cover it mid-read
#   LOW_MQ   the alt reads are MAPQ 20 among MAPQ 60 reference reads
# ---------------------------------------------------------------------------------------------------------------------------
CLEAN, LOW_BQ, READ_END, LOW_MQ = 1050, 1060, 1030, 1070


def planted_reads():
    rng = np.random.default_rng(2907)
    reads = []
    for k in range(400):
        group = k // 40  # 0 .. 3 carry one planted alt each, 4 .. 9 are reference reads everywhere
        start = 1000 + k % 21
        if group == 2:
            start = READ_END - k % 3
        seq, qual = ["A"] * 100, [40] * 100
        if group < 4:
            at = (CLEAN, LOW_BQ, READ_END, LOW_MQ)[group] - start
            seq[at] = "C"
            if group == 1:
                qual[at] = 20 + k % 2
        reads.append(read(0, start - 1, "100M", rng, flag=0x10 * (k & 1), mapq=20 if group == 3 else 60, seq="".join(seq), qual=qual))
    return sorted(reads, key=lambda r: r["pos"])


def test_four_planted_calls_end_to_end(tmp_path):
    reads = planted_reads()
    lines = [("chr1", CLEAN, "A", "C"), ("chr1", LOW_BQ, "A", "."), ("chr1", READ_END, "A", "C"), ("chr1", LOW_MQ, "A", ".")]
    ev, hist, res = model_files(reads, lines, 20, 20, 4, 3.0)
    got = [l.split("\t") for l in ev.splitlines()]
    assert [g[-1] for g in got] == ["PASS", "LOW_BQ", "READ_END", "LOW_MQ"]  # the model's verdicts, before the device is touched
    assert [g[3:6] for g in got] == [["C", "360", "40"]] * 4 and res.stats == (400, 1600)
    helpers.write_bam(tmp_path / "P.bam", REFS, reads)
    write_vcf(tmp_path / "v.txt", lines)
    r = run_re(f"vcf={tmp_path}/v.txt", f"bam={tmp_path}/P.bam", f"out={tmp_path}")
    assert r.returncode == 0, r.stdout + r.stderr
    assert (tmp_path / "P.EVIDENCE.txt").read_text() == ev
    assert (tmp_path / "P.EVIDENCE.HIST.txt").read_text() == hist
