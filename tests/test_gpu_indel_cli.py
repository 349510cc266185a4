"""computeIndelCounts on the GPU (BAM -> .INDEL.PILEUP.ASEQ + .INDEL.LENGTHS.txt; ampli_pileup_indel_count over computeCounts' batch
loop) against the model of tests/indel_model.py on the same synthetic BAM files, byte for byte; the refbases= table; a corrupt file;
and an end-to-end cohort whose indel count files go through the two drop-in command lines and come out as what the CPU oracle
(oracle/pyoracle.py) computes from the model's counts."""
import os
import re
import subprocess

import numpy as np
import pytest

from amplisolve_amd.hostio import HostCohort, read_error_table
from oracle import pyoracle as orc
from tests import helpers
from tests import indel_model as im
from tests.pileup_model import read

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "amplisolve_amd", "bin")
REFS = [("chr1", 100000), ("chr8", 50000), ("chrX", 30000), ("chrUn", 5000)]
AMPS = [(0, 1000, 1120), (0, 1100, 1230), (1, 5000, 5100), (2, 200, 330), (2, 29950, 29999)]
ASEQ_HEADER = "chr\tpos\tdbsnp\tMAF\tref\talt\tA\tC\tG\tT\tRD\tArs\tCrs\tGrs\tTrs\n"


def positions():
    """the VCF-like list: every position of the amplicons in order (overlaps -> positions listed twice), plus a chromosome the BAM does
    not know and an uncovered stretch"""
    names = [n for n, _ in REFS]
    lines = [(names[r], p, ".") for r, s, e in AMPS for p in range(s, e + 1)]
    return lines + [("chr22", p, ".") for p in range(10, 15)] + [("chr8", p, "rs1") for p in range(40000, 40005)]


def write_vcf(path, lines):
    with open(path, "w") as f:
        for c, p, i in lines:
            f.write(f"{c}\t{p}\t{i}\tN\t.\t.\t.\t.\n")


def model_files(reads, lines, mbq, mrq, mdc):
    """(ASEQ text, LENGTHS text, Result) the command must write for `reads` on the listed positions: the model's counts, formatted here"""
    names = [n for n, _ in REFS]
    known = [(names.index(c), p) for c, p, _ in lines if c in names]
    keys = im.make_keys(known)
    res = im.count(reads, keys, mbq, mrq) if reads else im.Result(np.zeros((len(keys), 8), np.int64), np.zeros((len(keys), 2, im.BINS), np.int64), (0, 0))
    index = {int(k): i for i, k in enumerate(keys.tolist())}
    aseq, lens, seen = [ASEQ_HEADER], [], set()
    for c, p, i in lines:
        k = index.get((names.index(c) << 32) | p) if c in names else None
        row = res.counts[k].tolist() if k is not None else [0] * 8
        rd = row[0] + row[1] + row[2]
        if rd >= mdc:
            aseq.append(f"{c}\t{p}\t{i}\t.\tA\t.\t{row[0]}\t{row[1]}\t{row[2]}\t{row[3]}\t{rd}\t{row[4]}\t{row[5]}\t{row[6]}\t{row[7]}\n")
        if k is not None and k not in seen:
            seen.add(k)
            lens += [f"{c}\t{p}\t{'DEL' if kind else 'INS'}\t{b + 1}\t{res.lengths[k, kind, b]}\n" for kind in (0, 1) for b in range(im.BINS) if res.lengths[k, kind, b]]
    return "".join(aseq), "".join(lens), res


def run_ci(*args, env=None, **kw):
    return subprocess.run([f"{BIN}/computeIndelCounts", *[str(a) for a in args]], capture_output=True, text=True, timeout=300,
                          env=dict(os.environ, AMPLISOLVE_STRICT_EXIT="1", **(env or {})), **kw)


@pytest.mark.parametrize("seed,n_reads,mbq,mrq,mdc,batch", [(1, 3000, 20, 20, 20, None), (2, 1500, 0, 0, 0, "70000"), (3, 2500, 21, 40, 0, "70000"), (4, 600, 30, 5, 20, None)])
def test_the_files_equal_the_model_byte_for_byte(tmp_path, seed, n_reads, mbq, mrq, mdc, batch):
    rng = np.random.default_rng(seed)
    reads = im.roughen(rng, helpers.random_amplicon_reads(rng, REFS, AMPS, n_reads, odd_ops=0.3))
    helpers.write_bam(tmp_path / "S1.bam", REFS, reads, rng=rng, max_block=20000)
    lines = positions()
    write_vcf(tmp_path / "v.txt", lines)
    out = tmp_path / "out"
    out.mkdir()
    r = run_ci(f"vcf={tmp_path}/v.txt", f"bam={tmp_path}/S1.bam", "threads=3", f"mbq={mbq}", f"mrq={mrq}", f"mdc={mdc}", f"out={out}",
               env={"AMPLISOLVE_BAM_BATCH_BYTES": batch} if batch else None)  # many small batches: records and even the header span batch boundaries
    assert r.returncode == 0, r.stdout + r.stderr
    aseq, lens, res = model_files(reads, lines, mbq, mrq, mdc)
    assert (out / "S1.INDEL.PILEUP.ASEQ").read_text() == aseq
    assert (out / "S1.INDEL.LENGTHS.txt").read_text() == lens
    assert sorted(os.listdir(out)) == ["S1.INDEL.LENGTHS.txt", "S1.INDEL.PILEUP.ASEQ"]  # no temporary file stays
    assert res.counts[:, 1].sum() > 20 and res.counts[:, 2].sum() > 20 and len(lens.splitlines()) > 20
    assert f"{len(reads)} alignment records (0 malformed), {res.stats[0]} kept (mrq {mrq}), {res.stats[1]} junctions counted (mbq {mbq}) over {len(lines)} listed positions" in r.stdout
    if mdc == 0:  # every listed position, the unknown chromosome and the duplicates included
        assert len(aseq.splitlines()) == 1 + len(lines)
    else:
        assert 100 < len(aseq.splitlines()) < len(lines)


def test_the_refbases_table_and_an_empty_file(tmp_path):
    lines = positions()
    write_vcf(tmp_path / "v.txt", lines)
    helpers.write_bam(tmp_path / "E.bam", REFS, [])
    r = run_ci(f"vcf={tmp_path}/v.txt", f"bam={tmp_path}/E.bam", "mdc=0", f"refbases={tmp_path}/ref.txt", f"out={tmp_path}")
    assert r.returncode == 0, r.stdout + r.stderr
    assert (tmp_path / "ref.txt").read_text() == "".join(f"{c}\t{p}\tA\n" for c, p, _ in lines)
    got = (tmp_path / "E.INDEL.PILEUP.ASEQ").read_text().splitlines()
    assert len(got) == 1 + len(lines) and all(l.split("\t")[4:] == ["A", "."] + ["0"] * 9 for l in got[1:])
    assert (tmp_path / "E.INDEL.LENGTHS.txt").read_text() == ""
    assert not [n for n in os.listdir(tmp_path) if ".tmp" in n]
    # without the key no table is written
    (tmp_path / "o2").mkdir()
    r = run_ci(f"vcf={tmp_path}/v.txt", f"bam={tmp_path}/E.bam", "mdc=0", f"out={tmp_path}/o2")
    assert r.returncode == 0 and sorted(os.listdir(tmp_path / "o2")) == ["E.INDEL.LENGTHS.txt", "E.INDEL.PILEUP.ASEQ"]


def test_a_corrupt_bam_leaves_no_file(tmp_path):
    rng = np.random.default_rng(21)
    reads = helpers.random_amplicon_reads(rng, REFS, AMPS, 800)
    helpers.write_bam(tmp_path / "C.bam", REFS, reads, rng=rng, max_block=5000, corrupt_block_size=(400, 0x7FFFFFFF))
    write_vcf(tmp_path / "v.txt", positions())
    (tmp_path / "o").mkdir()
    r = run_ci(f"vcf={tmp_path}/v.txt", f"bam={tmp_path}/C.bam", "mdc=0", f"refbases={tmp_path}/o/ref.txt", f"out={tmp_path}/o")
    assert r.returncode != 0 and "computeIndelCounts: " in r.stdout and "corrupt BAM record at uncompressed byte" in r.stdout
    assert os.listdir(tmp_path / "o") == []
    # a file cut off inside a record
    helpers.write_bam(tmp_path / "T.bam", REFS, reads[:50])
    raw = (tmp_path / "T.bam").read_bytes()
    (tmp_path / "T.bam").write_bytes(raw[:len(raw) // 2])
    r = run_ci(f"vcf={tmp_path}/v.txt", f"bam={tmp_path}/T.bam", "mdc=0", f"out={tmp_path}/o")
    assert r.returncode != 0 and os.listdir(tmp_path / "o") == []


# ---------------------------------------------------------------------------------------------------------------------------
# the end-to-end cohort
# ---------------------------------------------------------------------------------------------------------------------------
# Two amplicons of 60 columns, ~2000 full-length reads each per file, both strands alike.  HOMOPOLYMER: a junction where every file
# shows a 1-bp deletion in about 2 % of its reads; DELETION: a 15-bp deletion and INSERTION: a 3-bp insertion in about 5 % of the
# tumour's reads, absent from the normals.  The numbers below were fixed after the CPU oracle, run on the model's counts, gave
# exactly the calls this test asserts.  Its scores (Q forward, Q reverse; the gate is 5) for the tumour at the three junctions:
#   chr1:1040 A>G (the 15-bp deletion)   Q = COHORT_SCORES["deletion"]
#   chr8:5030 A>C (the 3-bp insertion)   Q = COHORT_SCORES["insertion"]
#   chr1:1020 A>G (the homopolymer)      not called: COHORT_SCORES["homopolymer"]
E2E_AMPS = (("chr1", 0, 1000), ("chr8", 1, 5000))
E2E_LEN = 60
HOMOPOLYMER, DELETION, INSERTION = ("chr1", 1020), ("chr1", 1040), ("chr8", 5030)
N_NORMALS = 8
# (100 is the scorer's ceiling: 50 of 1000 reads per strand against the default rate 0.002; the homopolymer junction shows 22 of 1000 per
# strand against the panel's 0.02175)
COHORT_SCORES = {"deletion": (100.0, 100.0), "insertion": (100.0, 100.0), "homopolymer": (2.949376, 2.949376)}


def cohort_reads(sample):
    """the reads of normal 0..7 or of the tumour (sample = N_NORMALS): per amplicon 1000 forward and 1000 reverse reads, the events dealt
    to fixed numbers of them"""
    rng = np.random.default_rng(4100 + sample)
    tumour = sample == N_NORMALS
    homo = 20 + (sample * 3) % 5 - 2  # 18..22 of 1000 per strand: about 2 %
    seq, qual = "ACGT" * 20, [35] * 80
    out = []
    for _, ref_id, start in E2E_AMPS:
        for strand in (0, 1):
            for k in range(1000):
                cigar = f"{E2E_LEN}M"
                if ref_id == 0 and k < homo:
                    cigar = "21M1D38M"
                elif ref_id == 0 and tumour and 100 <= k < 150:
                    cigar = "41M15D4M"
                elif ref_id == 1 and tumour and 100 <= k < 150:
                    cigar = "31M3I29M"
                n = sum(int(x) for x, o in re.findall(r"(\d+)([MI])", cigar))
                out.append(read(ref_id, start - 1, cigar, rng, flag=0x10 * strand, seq=seq[:n], qual=qual[:n], name=f"s{sample}"))
    out.sort(key=lambda r: (r["ref_id"], r["pos"]))
    return out


def cohort_lines():
    return [(c, p, ".") for c, _, s in E2E_AMPS for p in range(s, s + E2E_LEN)]


def oracle_outputs(d):
    """(error table text, expected Summary rows) of the CPU oracle on the count files under d/N and d/T, the reference bases from d/ref.txt"""
    co = HostCohort(f"{d}/p.bed", f"{d}/N", refbases_file=f"{d}/ref.txt")
    acc = orc.error_reduce(co.recs, co.P, 0.002, 100, E=co.E, dup_off=co.dup_off)
    assert acc["order_sensitive"] == 0
    fin = orc.error_finalize(acc)
    table = f"{d}/oracle_table.txt"
    co.write_error_table(fin["rate"], fin["code"], fin["germ_val"].astype(np.float32), fin["germ_present"], table)
    ct = HostCohort(table, f"{d}/T", is_error_table=True, keep_line_no=True)
    ref, thr = read_error_table(table)
    exp = orc.poisson_call(ct.recs, ct.P, thr, ref, 100, E=ct.E, ext_pos=ct.ext_pos)
    want = []
    for t, name in enumerate(ct.names):
        for _, r in sorted((ct.line_no[t, r], r) for r in range(ct.P + ct.E) if exp["call_mask"][t, r]):
            c, x = ct.position(r if r < ct.P else ct.ext_pos[r - ct.P])
            want += [(name, c, str(x), f"A->{'ACGT'[a]}", float(exp["q"][t, r, a, 0]), float(exp["q"][t, r, a, 1])) for a in range(4) if exp["call_mask"][t, r] >> a & 1]
    q = {(ct.position(p)[0], int(ct.position(p)[1])): exp["q"][0, p] for p in range(ct.P)}
    return open(table).read(), want, q


def write_model_cohort(d):
    """the model's count files of the cohort under d/N and d/T, the panel and the reference bases: what computeIndelCounts must write"""
    lines = cohort_lines()
    for sub in ("N", "T"):
        os.makedirs(f"{d}/{sub}", exist_ok=True)
    texts = {}
    for s in range(N_NORMALS + 1):
        name = f"N{s}" if s < N_NORMALS else "TUM"
        aseq, lens, _ = model_files(cohort_reads(s), lines, 20, 20, 20)
        texts[name] = (aseq, lens)
        with open(f"{d}/{'N' if s < N_NORMALS else 'T'}/{name}.INDEL.PILEUP.ASEQ", "w") as f:
            f.write(aseq)
    with open(f"{d}/p.bed", "w") as f:
        f.write("".join(f"{c}\t{s}\t{s + E2E_LEN - 1}\n" for c, _, s in E2E_AMPS))
    with open(f"{d}/ref.txt", "w") as f:
        f.write("".join(f"{c}\t{p}\tA\n" for c, p, _ in lines))
    return texts


def test_end_to_end_cohort_through_both_command_lines(tmp_path):
    model = tmp_path / "model"
    model.mkdir()
    texts = write_model_cohort(str(model))
    table, want, q = oracle_outputs(str(model))
    # the oracle's verdict on the model's counts: the two planted junctions are called, the homopolymer junction is not
    assert [w[:4] for w in want] == [("TUM.INDEL", "chr1", "1040", "A->G"), ("TUM.INDEL", "chr8", "5030", "A->C")]
    for key, site, a in (("deletion", DELETION, 2), ("insertion", INSERTION, 1), ("homopolymer", HOMOPOLYMER, 2)):
        print(key, q[site][a].tolist())
        assert np.allclose(q[site][a], COHORT_SCORES[key], rtol=1e-6), (key, q[site][a])
    # files -> computeIndelCounts, all nine at once: every run writes the same refbases table into place
    d = tmp_path / "run"
    for sub in ("bam", "N", "T"):
        (d / sub).mkdir(parents=True)
    lines = cohort_lines()
    write_vcf(d / "v.txt", lines)
    procs = []
    for s in range(N_NORMALS + 1):
        name = f"N{s}" if s < N_NORMALS else "TUM"
        helpers.write_bam(d / "bam" / f"{name}.bam", REFS, cohort_reads(s), max_block=60000, level=1)
        procs.append(subprocess.Popen([f"{BIN}/computeIndelCounts", f"vcf={d}/v.txt", f"bam={d}/bam/{name}.bam", "mbq=20", "mrq=20", "mdc=20", f"refbases={d}/ref.txt",
                                       f"out={d}/{'N' if s < N_NORMALS else 'T'}"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
                                      env=dict(os.environ, AMPLISOLVE_STRICT_EXIT="1")))
    for p in procs:
        out, _ = p.communicate(timeout=300)
        assert p.returncode == 0, out
    for name, (aseq, lens) in texts.items():
        sub = "T" if name == "TUM" else "N"
        assert (d / sub / f"{name}.INDEL.PILEUP.ASEQ").read_text() == aseq
        assert (d / sub / f"{name}.INDEL.LENGTHS.txt").read_text() == lens
    assert (d / "ref.txt").read_text() == (model / "ref.txt").read_text() and not [n for n in os.listdir(d) if ".tmp" in n]
    assert "chr1\t1040\tDEL\t15\t100\n" in texts["TUM"][1] and "chr8\t5030\tINS\t3\t100\n" in texts["TUM"][1]  # the called deletion is the 15-bp one
    # -> the two drop-in command lines, the reference bases from the written table
    env = dict(os.environ, AMPLISOLVE_STRICT_EXIT="1", AMPLISOLVE_REFBASES_FILE=f"{d}/ref.txt")
    (d / "p.bed").write_text((model / "p.bed").read_text())
    r = subprocess.run([f"{BIN}/AmpliSolveErrorEstimation", f"panel_design={d}/p.bed", "reference_genome=unused.fa", f"germline_dir={d}/N", "C_value=0.002",
                        "coverage_cutoff=100", "default_error=0.01", f"output_dir={d}/ee"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert (d / "ee" / "positionSpecificNoise_0.0020.txt").read_text() == table
    r = subprocess.run([f"{BIN}/AmpliSolveVariantCalling", f"errorFile={d}/ee/positionSpecificNoise_0.0020.txt", f"tumour_dir={d}/T", f"output_dir={d}/vc",
                        "coverage_cutoff=100", "p_value=0.05"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [l.split("\t") for l in (d / "vc" / "Summary_Variant_Info.txt").read_text().splitlines()][1:]
    assert len(rows) == len(want) == 2
    for got, w in zip(rows, want):
        assert tuple(got[:4]) == w[:4] and got[14] == f"{w[4]:.4g}" and got[15] == f"{w[5]:.4g}", (got, w)
