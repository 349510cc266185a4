"""computeAmpliconCounts on the GPU (BAM + BED -> .AMPLICON.PILEUP.ASEQ, .AMPLICON.READS.txt, .AMPLICON.OVERLAPS.txt and the layers;
ampli_pileup_amplicon_count over computeCounts' batch loop, ampli_amplicon_layers behind it) against the model of
tests/amplicon_count_model.py on the same synthetic BAM files, byte for byte; a corrupt and a truncated file; a BAM on which the
command must write computeCounts' own lines; and, end to end, AmpliSolvePairedComparison on the two layers of a panel with one overlap,
which must tell a variant that both amplicons show from an artefact that only the first one shows."""
import os
import subprocess

import numpy as np
import pytest

from tests import amplicon_count_model as am
from tests import helpers
from tests import paired_model as pd
from tests.pileup_model import read

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "amplisolve_amd", "bin")
REFS = [("chr1", 100000), ("chr8", 50000), ("chrX", 30000), ("chrUn", 5000)]
NAMES = [n for n, _ in REFS]
# BED rows in file order: overlapping, nested, repeated, on a chromosome the BAM does not know, and a header line
BED = [("chrX", 200, 330), ("chr1", 1100, 1230), ("chr1", 1000, 1124), ("chr22", 10, 90), ("chr8", 5000, 5100), ("chr8", 5000, 5100), ("chr1", 1110, 1150),
       ("chrX", 29950, 29999), ("chr8", 5080, 5200)]
ASEQ_HEADER = "chr\tpos\tdbsnp\tMAF\tref\talt\tA\tC\tG\tT\tRD\tArs\tCrs\tGrs\tTrs\n"


def write_bed(path, rows=BED, header=True):
    with open(path, "w") as f:
        if header:
            f.write("chrom\tstart\tend\tname\tscore\tgene\n")
        for k, (c, s, e) in enumerate(rows):
            f.write(f"{c}\t{s}\t{e}\tamp{k}\t0\tGENE{k % 4}\n")


def positions(rows=BED):
    """the VCF-like list: every position of every BED row in order (overlaps -> positions listed twice), plus an uncovered stretch"""
    return [(c, p, f"rs{p % 7}", "ACGT"[p % 4], "ACGT"[(p + 1) % 4]) for c, s, e in rows for p in range(s, e + 1)] + [("chr8", p, ".", "N", ".") for p in range(40000, 40005)]


def write_vcf(path, lines):
    with open(path, "w") as f:
        for c, p, i, r, a in lines:
            f.write(f"{c}\t{p}\t{i}\t{r}\t{a}\t.\t.\t.\n")


def aseq_line(c, p, i, r, a, row):
    row = [int(x) for x in row]
    return f"{c}\t{p}\t{i}\t.\t{r}\t{a}\t{row[0]}\t{row[1]}\t{row[2]}\t{row[3]}\t{sum(row[:4])}\t{row[4]}\t{row[5]}\t{row[6]}\t{row[7]}\n"


def model_files(reads, rows, lines, mbq, mrq, mdc, min_overlap, header=True):
    """{file name behind "<bam name>.": text} the command must write, and the model's Result: the model's integers, formatted here"""
    known = [k for k, (c, _, _) in enumerate(rows) if c in NAMES]
    amps = am.make_amplicons([(NAMES.index(rows[k][0]), rows[k][1], rows[k][2]) for k in known])
    res = am.count(reads, amps, mbq, mrq, min_overlap) if reads else am.count(([0] * 16, []), amps, mbq, mrq, min_overlap)
    keys = np.asarray([am.key_of(NAMES.index(c), p) for c, p, *_ in lines if c in NAMES], np.uint64)
    lay = am.layers(res.counts, amps, keys, 2)
    sorted_of = {known[int(r)]: a for a, r in enumerate(amps.row_of.tolist())}
    files = {"AMPLICON.PILEUP.ASEQ": [ASEQ_HEADER], "AMPLICON.OVERLAPS.txt": [], "AMP1.PILEUP.ASEQ": [ASEQ_HEADER], "AMP2.PILEUP.ASEQ": [ASEQ_HEADER]}
    slot = 0
    for c, p, i, r, a in lines:
        if c not in NAMES:
            if 0 >= mdc:
                files["AMPLICON.PILEUP.ASEQ"].append(aseq_line(c, p, i, r, a, [0] * 8))
            continue
        if lay.total[slot, :4].sum() >= mdc:
            files["AMPLICON.PILEUP.ASEQ"].append(aseq_line(c, p, i, r, a, lay.total[slot]))
        for l in (0, 1):
            if lay.layer_amp[l, slot] >= 0 and lay.layers[l, slot, :4].sum() >= mdc:
                files[f"AMP{l + 1}.PILEUP.ASEQ"].append(aseq_line(c, p, i, r, a, lay.layers[l, slot]))
        cover = am.covering(amps, keys[slot])
        if len(cover) >= 2:
            for a_ in cover:
                rec = res.counts[int(amps.amp_off[a_]) + p - int(amps.first[a_])]
                files["AMPLICON.OVERLAPS.txt"].append(f"{c}\t{p}\tamp{known[int(amps.row_of[a_])]}\t" + "\t".join(str(int(x)) for x in rec) + "\n")
        slot += 1
    rd = ["chrom\t-1\t-1\t.\t.\t0\t0\n"] if header else []  # the header line is a BED row like any other: reported, with zeros
    for k, (c, s, e) in enumerate(rows):
        fw, rv = res.amp_reads[sorted_of[k]].tolist() if k in sorted_of else (0, 0)
        rd.append(f"{c}\t{s}\t{e}\tamp{k}\tGENE{k % 4}\t{fw}\t{rv}\n")
    st = res.stats
    rd.append(f"#kept\t{st[0]}\n#assigned\t{st[1]}\n#off_target\t{st[0] - st[1]}\n#bases_counted\t{st[2]}\n#bases_clipped\t{st[3]}\n")
    files["AMPLICON.READS.txt"] = rd
    return {k: "".join(v) for k, v in files.items()}, res


def run(exe, *args, env=None, **kw):
    e = dict(os.environ, AMPLISOLVE_STRICT_EXIT="1", **(env or {}))
    e.pop("AMPLISOLVE_LIST_DIR_AS", None)
    return subprocess.run([f"{BIN}/{exe}", *[str(a) for a in args]], capture_output=True, text=True, timeout=300, env=e, **kw)


@pytest.mark.parametrize("seed,n_reads,mbq,mrq,mdc,min_overlap", [(1, 3000, 20, 20, 20, 50), (2, 1500, 0, 0, 0, 1), (3, 2500, 21, 40, 0, 80), (4, 600, 30, 5, 20, 100)])
def test_the_files_equal_the_model_byte_for_byte(tmp_path, seed, n_reads, mbq, mrq, mdc, min_overlap):
    rng = np.random.default_rng(seed)
    targets = [(NAMES.index(c), s, e) for c, s, e in BED if c in NAMES] + [(1, 20000, 20030), (3, 100, 200)]  # and reads that belong to no BED row
    reads = helpers.random_amplicon_reads(rng, REFS, targets, n_reads, odd_ops=0.3)
    helpers.write_bam(tmp_path / "S1.bam", REFS, reads, rng=rng, max_block=20000)
    lines = positions()
    write_vcf(tmp_path / "v.txt", lines)
    write_bed(tmp_path / "p.bed")
    out, lay = tmp_path / "out", tmp_path / "layers"
    out.mkdir()
    lay.mkdir()
    r = run("computeAmpliconCounts", f"vcf={tmp_path}/v.txt", f"bam={tmp_path}/S1.bam", f"bed={tmp_path}/p.bed", "threads=3", f"mbq={mbq}", f"mrq={mrq}", f"mdc={mdc}",
            f"min_overlap={min_overlap}", f"layers={lay}", f"out={out}", env={"AMPLISOLVE_BAM_BATCH_BYTES": "70000"})  # many small batches
    assert r.returncode == 0, r.stdout + r.stderr
    want, res = model_files(reads, BED, lines, mbq, mrq, mdc, min_overlap)
    for name in ("AMPLICON.PILEUP.ASEQ", "AMPLICON.READS.txt", "AMPLICON.OVERLAPS.txt"):
        assert (out / f"S1.{name}").read_text() == want[name], name
    for name in ("AMP1.PILEUP.ASEQ", "AMP2.PILEUP.ASEQ"):
        assert (lay / f"S1.{name}").read_text() == want[name], name
    assert (lay / "S1.pairs.txt").read_text() == "S1.AMP1\tS1.AMP2\n"
    assert sorted(os.listdir(out)) == ["S1.AMPLICON.OVERLAPS.txt", "S1.AMPLICON.PILEUP.ASEQ", "S1.AMPLICON.READS.txt"]  # no temporary file stays
    assert sorted(os.listdir(lay)) == ["S1.AMP1.PILEUP.ASEQ", "S1.AMP2.PILEUP.ASEQ", "S1.pairs.txt"]
    st = res.stats
    # what the stream holds, on the model: off-target reads, clipped columns (none at min_overlap 100: such a read lies inside its amplicon)
    assert st[0] > st[1] > 50 and (st[3] > 100) == (min_overlap < 100) and len(want["AMPLICON.OVERLAPS.txt"].splitlines()) > 200
    assert f"{len(reads)} alignment records (0 malformed), {st[0]} kept (mrq {mrq}), {st[1]} assigned" in r.stdout
    if mdc == 0:  # every listed position, the unknown chromosome and the duplicates included
        assert len(want["AMPLICON.PILEUP.ASEQ"].splitlines()) == 1 + len(lines) and len(want["AMP2.PILEUP.ASEQ"].splitlines()) > 100


def test_an_empty_file_and_no_layers(tmp_path):
    lines = positions()
    write_vcf(tmp_path / "v.txt", lines)
    write_bed(tmp_path / "p.bed", header=False)
    helpers.write_bam(tmp_path / "E.bam", REFS, [])
    r = run("computeAmpliconCounts", f"vcf={tmp_path}/v.txt", f"bam={tmp_path}/E.bam", f"bed={tmp_path}/p.bed", "mdc=0", f"out={tmp_path}")
    assert r.returncode == 0, r.stdout + r.stderr
    want, _ = model_files([], BED, lines, 20, 20, 0, 50, header=False)
    for name in ("AMPLICON.PILEUP.ASEQ", "AMPLICON.READS.txt", "AMPLICON.OVERLAPS.txt"):
        assert (tmp_path / f"E.{name}").read_text() == want[name], name
    assert not [n for n in os.listdir(tmp_path) if ".tmp" in n or ".AMP1." in n or "pairs" in n]


def test_a_corrupt_and_a_truncated_bam_leave_no_file(tmp_path):
    rng = np.random.default_rng(21)
    reads = helpers.random_amplicon_reads(rng, REFS, [(0, 1000, 1124), (1, 5000, 5100)], 800)
    helpers.write_bam(tmp_path / "C.bam", REFS, reads, rng=rng, max_block=5000, corrupt_block_size=(400, 0x7FFFFFFF))
    write_vcf(tmp_path / "v.txt", positions())
    write_bed(tmp_path / "p.bed")
    (tmp_path / "o").mkdir()
    (tmp_path / "l").mkdir()
    common = (f"vcf={tmp_path}/v.txt", f"bed={tmp_path}/p.bed", "mdc=0", f"layers={tmp_path}/l", f"out={tmp_path}/o")
    r = run("computeAmpliconCounts", f"bam={tmp_path}/C.bam", *common)
    assert r.returncode != 0 and "computeAmpliconCounts: " in r.stdout and "corrupt BAM record at uncompressed byte" in r.stdout
    assert os.listdir(tmp_path / "o") == [] and os.listdir(tmp_path / "l") == []
    helpers.write_bam(tmp_path / "T.bam", REFS, reads[:50])  # a file cut off inside a record
    raw = (tmp_path / "T.bam").read_bytes()
    (tmp_path / "T.bam").write_bytes(raw[:len(raw) // 2])
    r = run("computeAmpliconCounts", f"bam={tmp_path}/T.bam", *common)
    assert r.returncode != 0 and os.listdir(tmp_path / "o") == [] and os.listdir(tmp_path / "l") == []


def test_reads_inside_disjoint_amplicons_give_computeCounts_lines(tmp_path):
    """every read inside its amplicon, no position under two amplicons: nothing is clipped, nothing is off-target, and the totals are
    the pooled counts -- the file equals computeCounts' of the same BAM, line for line"""
    rng = np.random.default_rng(8)
    rows = [("chr1", 1000, 1120), ("chr8", 5000, 5100), ("chr1", 1121, 1200)]
    reads = []
    for _ in range(1500):
        c, s, e = rows[int(rng.integers(len(rows)))]
        n = int(rng.integers(20, e - s - 10))
        at = int(rng.integers(s, e - n - 4))
        cigar = f"{n}M" if rng.random() < 0.6 else f"3S{n // 2}M2I{n - n // 2}M" if rng.random() < 0.5 else f"{n // 2}M4D{n - n // 2}M5S"
        reads.append(read(NAMES.index(c), at - 1, cigar, rng, flag=0x10 * int(rng.integers(2)), mapq=int(rng.choice([5, 20, 60]))))
    reads.sort(key=lambda r: (r["ref_id"], r["pos"]))
    helpers.write_bam(tmp_path / "D.bam", REFS, reads, rng=rng, max_block=20000)
    lines = positions(rows)
    write_vcf(tmp_path / "v.txt", lines)
    write_bed(tmp_path / "p.bed", rows, header=False)
    for sub in ("pooled", "amp"):
        (tmp_path / sub).mkdir()
    common = (f"vcf={tmp_path}/v.txt", f"bam={tmp_path}/D.bam", "mbq=30", "mrq=20", "mdc=20")
    r = run("computeCounts", *common, f"out={tmp_path}/pooled")
    assert r.returncode == 0, r.stdout + r.stderr
    r = run("computeAmpliconCounts", *common, f"bed={tmp_path}/p.bed", "min_overlap=100", f"out={tmp_path}/amp")
    assert r.returncode == 0, r.stdout + r.stderr
    pooled = (tmp_path / "pooled" / "D.PILEUP.ASEQ").read_text()
    assert (tmp_path / "amp" / "D.AMPLICON.PILEUP.ASEQ").read_text() == pooled and len(pooled.splitlines()) > 200
    assert "#off_target\t0\n" in (tmp_path / "amp" / "D.AMPLICON.READS.txt").read_text() and "#bases_clipped\t0\n" in (tmp_path / "amp" / "D.AMPLICON.READS.txt").read_text()
    assert (tmp_path / "amp" / "D.AMPLICON.OVERLAPS.txt").read_text() == ""


# ---------------------------------------------------------------------------------------------------------------------------
# end to end: the two layers through AmpliSolvePairedComparison
# ---------------------------------------------------------------------------------------------------------------------------
Q_MIN, DEPTH_CUTOFF, MIN_VAF = 13, 100, 0.005
N_STRAND, N_ALT = 200, 60  # reads per amplicon and strand, and how many of them carry a planted base
SHARED_AT, ARTEFACT_AT = 1090, 1095  # both inside the overlap 1080 .. 1100 of the two amplicons


def test_paired_comparison_of_the_two_layers_tells_an_artefact_from_a_variant(tmp_path):
    # on the CPU first: the planted counts give these verdicts under the paired model at this q_min and depth_cutoff
    s_art = float(pd.pair_s(N_ALT, N_STRAND, 0, N_STRAND))
    s_shared = float(pd.pair_s(N_ALT, N_STRAND, N_ALT, N_STRAND))
    vaf = N_ALT / N_STRAND
    assert N_STRAND >= DEPTH_CUTOFF and pd.verdict(s_art, s_art, vaf, 0.0, Q_MIN, MIN_VAF) == "HIGHER_IN_A" and s_art >= Q_MIN + 1
    assert pd.verdict(s_shared, s_shared, vaf, vaf, Q_MIN, MIN_VAF) == "SHARED" and abs(s_shared) <= Q_MIN - 1
    refs = [("chr7", 100000)]
    rows = [("chr7", 1000, 1100), ("chr7", 1080, 1180)]
    rng = np.random.default_rng(5)
    reads = []
    for k, (_, s, e) in enumerate(rows):
        for rev in (0, 1):
            for i in range(N_STRAND):
                seq = ["A"] * (e - s + 1)
                if i < N_ALT:
                    seq[SHARED_AT - s] = "C"       # the variant: in the reads of both amplicons
                    if k == 0:
                        seq[ARTEFACT_AT - s] = "G"  # the artefact: in the reads of the first amplicon only
                reads.append(read(0, s - 1, f"{e - s + 1}M", rng, flag=0x10 * rev, seq="".join(seq), qual=[30] * (e - s + 1)))
    reads.sort(key=lambda r: r["pos"])
    helpers.write_bam(tmp_path / "S.bam", refs, reads, rng=rng)
    with open(tmp_path / "v.txt", "w") as f:
        for p in range(1000, 1181):
            f.write(f"chr7\t{p}\t.\tA\t.\n")
    (tmp_path / "p.bed").write_text("".join(f"{c}\t{s}\t{e}\tamp{k}\t0\tG\n" for k, (c, s, e) in enumerate(rows)))
    (tmp_path / "r.txt").write_text("".join(f"chr7\t{p}\tA\n" for p in list(range(1000, 1101)) + list(range(1080, 1181))))
    for sub in ("out", "layers"):
        (tmp_path / sub).mkdir()
    r = run("computeAmpliconCounts", f"vcf={tmp_path}/v.txt", f"bam={tmp_path}/S.bam", f"bed={tmp_path}/p.bed", "mdc=0", f"layers={tmp_path}/layers", f"out={tmp_path}/out")
    assert r.returncode == 0, r.stdout + r.stderr
    assert len((tmp_path / "layers" / "S.AMP1.PILEUP.ASEQ").read_text().splitlines()) == 1 + 181 and len((tmp_path / "layers" / "S.AMP2.PILEUP.ASEQ").read_text().splitlines()) == 1 + 21
    r = run("AmpliSolvePairedComparison", f"panel_design={tmp_path}/p.bed", "reference_genome=unused.fa", f"sample_dir={tmp_path}/layers", f"pairs={tmp_path}/layers/S.pairs.txt",
            f"depth_cutoff={DEPTH_CUTOFF}", f"q_min={Q_MIN}", f"min_vaf={MIN_VAF}", f"output_dir={tmp_path}/paired", env={"AMPLISOLVE_REFBASES_FILE": f"{tmp_path}/r.txt"}, cwd=tmp_path)
    assert r.returncode == 0, r.stdout[-800:] + r.stderr[-300:]
    cells = [l.split("\t") for l in (tmp_path / "paired" / "Paired_Cells.txt").read_text().splitlines()[1:]]
    verdicts = {(int(f[3]), f[4]): f[-1] for f in cells if (f[0], f[1]) == ("S.AMP1", "S.AMP2")}
    assert verdicts == {(ARTEFACT_AT, "A->G"): "HIGHER_IN_A", (SHARED_AT, "A->C"): "SHARED"}
    pairs_line = (tmp_path / "paired" / "Paired_Pairs.txt").read_text().splitlines()[1]
    assert pairs_line.startswith("S.AMP1\tS.AMP2\t") and pairs_line.endswith("\t1\t0\t1\t0")  # one HIGHER_IN_A, one SHARED, nothing else listed
