"""What AmpliSolvePairedComparison refuses before it opens the device, as tests/test_cli_refusals.py holds the other command lines to it:
a wrong number of tokens (the usage text), every bad number, AMPLISOLVE_WORLD_SIZE=2, and every fault of the list of pairs -- a file
that cannot be read, a malformed line, a file paired with itself, an unknown name, an empty list.  The exit status is 1, stdout is
exactly the text below, stderr is empty and no output directory appears.  None of these runs reaches the device."""
from tests.test_cli_refusals import ORDER, _refused, _run

EXE = "AmpliSolvePairedComparison"
TOKENS = ["panel_design=p.bed", "reference_genome=unused.fa", "sample_dir=S", "pairs=pairs.txt", "depth_cutoff=100", "q_min=13", "min_vaf=0.005", "output_dir=o"]
USAGE = ("Usage:\n\tAmpliSolvePairedComparison panel_design=<bed> reference_genome=<fasta> sample_dir=<dir> pairs=<file> depth_cutoff=<int> "
         "q_min=<float> min_vaf=<float> output_dir=<dir>" + ORDER +
         " (usual values: depth_cutoff=100 q_min=13 min_vaf=0.005; pairs lists nameA<TAB>nameB per line).\n")
BAD = [("depth_cutoff", "-1", "depth_cutoff must be an integer >= 0, got '-1'"),
       ("depth_cutoff", "", "depth_cutoff must be an integer >= 0, got ''"),
       ("depth_cutoff", "1e2", "depth_cutoff must be an integer >= 0, got '1e2'"),
       ("depth_cutoff", "2.5", "depth_cutoff must be an integer >= 0, got '2.5'"),
       ("q_min", "0", "q_min must be a number in (0, 100], got '0'"),
       ("q_min", "-5", "q_min must be a number in (0, 100], got '-5'"),
       ("q_min", "100.5", "q_min must be a number in (0, 100], got '100.5'"),
       ("q_min", "", "q_min must be a number in (0, 100], got ''"),
       ("q_min", "13q", "q_min must be a number in (0, 100], got '13q'"),
       ("q_min", "nan", "q_min must be a number in (0, 100], got 'nan'"),
       ("min_vaf", "-0.1", "min_vaf must be a number in [0, 1], got '-0.1'"),
       ("min_vaf", "1.5", "min_vaf must be a number in [0, 1], got '1.5'"),
       ("min_vaf", "x", "min_vaf must be a number in [0, 1], got 'x'"),
       ("min_vaf", "inf", "min_vaf must be a number in [0, 1], got 'inf'")]
HEADER = "chr\tpos\tdbsnp\tMAF\tref\talt\tA\tC\tG\tT\tRD\tArs\tCrs\tGrs\tTrs\n"
LISTS = [("TUM\tNORM\nTUM\n", "pairs: line 2 of 'pairs.txt' is not nameA<TAB>nameB"),
         ("TUM NORM\n", "pairs: line 1 of 'pairs.txt' is not nameA<TAB>nameB"),
         ("TUM\tNORM\tFOLLOW\n", "pairs: line 1 of 'pairs.txt' is not nameA<TAB>nameB"),
         ("\tNORM\n", "pairs: line 1 of 'pairs.txt' is not nameA<TAB>nameB"),
         ("TUM\t\n", "pairs: line 1 of 'pairs.txt' is not nameA<TAB>nameB"),
         ("TUM\tNORM\n\nFOLLOW\tNORM\n", "pairs: line 2 of 'pairs.txt' is not nameA<TAB>nameB"),
         ("TUM\tNORM\nNORM\tNORM\n", "pairs: line 2 pairs 'NORM' with itself"),
         ("TUM\tNORM\nTUM\tOTHER\n", "pairs: line 2 names 'OTHER', which is no count file of S"),
         ("tum\tNORM\n", "pairs: line 1 names 'tum', which is no count file of S"),
         ("TUM.PILEUP.ASEQ\tNORM\n", "pairs: line 1 names 'TUM.PILEUP.ASEQ', which is no count file of S"),
         ("", "pairs: 'pairs.txt' lists no pair")]


def test_usage(tmp_path):
    for n in (0, 4, 7):
        _refused(_run(EXE, TOKENS[:n], tmp_path), USAGE, tmp_path, n)
    _refused(_run(EXE, TOKENS + ["extra=1"], tmp_path), USAGE, tmp_path, "one token too many")


def test_every_bad_number(tmp_path):
    for key, bad, answer in BAD:
        t = [f"{key}={bad}" if x.startswith(key + "=") else x for x in TOKENS]
        assert t != TOKENS
        _refused(_run(EXE, t, tmp_path), f"{EXE} failed: {answer}\n", tmp_path, (key, bad))


def test_one_gpu(tmp_path):
    _refused(_run(EXE, TOKENS, tmp_path, AMPLISOLVE_WORLD_SIZE="2"), f"{EXE} failed: {EXE} runs on one GPU: AMPLISOLVE_WORLD_SIZE > 1 is not supported\n",
             tmp_path, "AMPLISOLVE_WORLD_SIZE=2")


def test_the_list_of_pairs(tmp_path):
    (tmp_path / "S").mkdir()
    for name in ("TUM", "NORM", "FOLLOW"):
        (tmp_path / "S" / f"{name}.PILEUP.ASEQ").write_text(HEADER)
    _refused(_run(EXE, TOKENS, tmp_path), f"{EXE} failed: pairs: cannot read 'pairs.txt'\n", tmp_path, "no list")
    for text, answer in LISTS:
        (tmp_path / "pairs.txt").write_text(text)
        _refused(_run(EXE, TOKENS, tmp_path), f"{EXE} failed: {answer}\n", tmp_path, text)
