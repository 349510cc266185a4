"""What AmpliSolveVariantMonitoring refuses before it opens the device, as tests/test_cli_refusals.py holds the other command lines to
it: a wrong number of tokens (the usage text), every bad number, AMPLISOLVE_WORLD_SIZE=2, and every fault of the two lists: a file that
cannot be read, a malformed or empty line, a bad position, a variant off the panel, a ref that is not the table's base, alt == ref, an
empty list, an unknown sample or list.  The exit status is 1, stdout is exactly the text below, stderr is empty and no output
directory appears.  None of these runs reaches the device."""
from tests.test_cli_refusals import ORDER, _refused, _run

EXE = "AmpliSolveVariantMonitoring"
TOKENS = ["errorFile=table.txt", "sample_dir=S", "variants=variants.txt", "assign=assign.txt", "coverage_cutoff=100", "q_min=20", "min_variants=5", "min_seen=2",
          "max_vaf=1", "controls=100", "seed=1", "output_dir=o"]
USAGE = ("Usage:\n\tAmpliSolveVariantMonitoring errorFile=<error table> sample_dir=<dir> variants=<file> assign=<file or -> coverage_cutoff=<int> "
         "q_min=<float> min_variants=<int> min_seen=<int> max_vaf=<float> controls=<int> seed=<int> output_dir=<dir>" + ORDER +
         " (usual values: coverage_cutoff=100 q_min=20 min_variants=5 min_seen=2 max_vaf=1 controls=100 seed=1).\n"
         "\tvariants: list<TAB>chrom<TAB>pos<TAB>ref<TAB>alt per line; assign: sample<TAB>list per line, or - for none.\n")
BAD = [("coverage_cutoff", "-1", "coverage_cutoff must be an integer >= 0, got '-1'"), ("coverage_cutoff", "x", "coverage_cutoff must be an integer >= 0, got 'x'"),
       ("q_min", "0", "q_min must be a number in (0, 100], got '0'"), ("q_min", "100.5", "q_min must be a number in (0, 100], got '100.5'"),
       ("q_min", "nan", "q_min must be a number in (0, 100], got 'nan'"), ("q_min", "", "q_min must be a number in (0, 100], got ''"),
       ("min_variants", "0", "min_variants must be an integer >= 1, got '0'"), ("min_variants", "2.5", "min_variants must be an integer >= 1, got '2.5'"),
       ("min_seen", "-1", "min_seen must be an integer >= 0, got '-1'"), ("min_seen", "", "min_seen must be an integer >= 0, got ''"),
       ("max_vaf", "1.5", "max_vaf must be a number in [0, 1], got '1.5'"), ("max_vaf", "-0.1", "max_vaf must be a number in [0, 1], got '-0.1'"),
       ("max_vaf", "x", "max_vaf must be a number in [0, 1], got 'x'"),
       ("controls", "-1", "controls must be an integer in [0, 1073741824], got '-1'"), ("controls", "1e3", "controls must be an integer in [0, 1073741824], got '1e3'"),
       ("seed", "", "seed must be an unsigned 64-bit integer, got ''"), ("seed", "-1", "seed must be an unsigned 64-bit integer, got '-1'"),
       ("seed", "18446744073709551616", "seed must be an unsigned 64-bit integer, got '18446744073709551616'")]
HEADER = "chr\tpos\tdbsnp\tMAF\tref\talt\tA\tC\tG\tT\tRD\tArs\tCrs\tGrs\tTrs\n"
TABLE = ("chrom\tposition\treference\tduplicate\tThres_A\tThres_C\tThres_G\tThres_T\tGerm_Max_A\tGerm_Max_C\tGerm_Max_G\tGerm_Max_T\n"
         "chr7\t100\tA\tNO\t-2_-2\t0.002000_0.002000\t0.002000_0.002000\t0.002000_0.002000\t-\t0\t0\t0\n"
         "chr7\t101\tG\tNO\t0.002000_0.002000\t0.002000_0.002000\t-2_-2\t0.002000_0.002000\t0\t0\t-\t0\n")
SHAPE = " of 'variants.txt' is not list<TAB>chrom<TAB>pos<TAB>ref<TAB>alt"
GOOD = "L1\tchr7\t100\tA\tC\n"
VARIANTS = [(GOOD + "L1\tchr7\t101\tG\n", "variants: line 2" + SHAPE), ("L1 chr7 100 A C\n", "variants: line 1" + SHAPE),
            (GOOD + "\n" + GOOD, "variants: line 2" + SHAPE), ("L1\tchr7\t100\tA\tC\textra\n", "variants: line 1" + SHAPE),
            ("\tchr7\t100\tA\tC\n", "variants: line 1" + SHAPE), ("L1\t\t100\tA\tC\n", "variants: line 1" + SHAPE),
            ("L1\tchr7\t1e2\tA\tC\n", "variants: line 1: pos must be a whole positive number, got '1e2'"),
            ("L1\tchr7\t0\tA\tC\n", "variants: line 1: pos must be a whole positive number, got '0'"),
            ("L1\tchr7\t-100\tA\tC\n", "variants: line 1: pos must be a whole positive number, got '-100'"),
            ("L1\tchr7\t\tA\tC\n", "variants: line 1: pos must be a whole positive number, got ''"),
            ("L1\tchr7\t100\tA\tN\n", "variants: line 1: ref and alt must each be one of A, C, G, T, got 'A' and 'N'"),
            ("L1\tchr7\t100\ta\tC\n", "variants: line 1: ref and alt must each be one of A, C, G, T, got 'a' and 'C'"),
            ("L1\tchr7\t100\tA\tCT\n", "variants: line 1: ref and alt must each be one of A, C, G, T, got 'A' and 'CT'"),
            ("L1\tchr7\t100\tA\tA\n", "variants: line 1: alt equals ref ('A')"),
            (GOOD + "L1\tchr7\t102\tA\tC\n", "variants: line 2: chr7:102 is not a position of the error table"),
            ("L1\tchr8\t100\tA\tC\n", "variants: line 1: chr8:100 is not a position of the error table"),
            (GOOD + "L2\tchr7\t101\tA\tC\n", "variants: line 2: ref 'A' is not the table's base 'G' at chr7:101"),
            ("", "variants: 'variants.txt' lists no variant")]
ASSIGN = [("PLA\tL1\nPLA\n", "assign: line 2 of 'assign.txt' is not sample<TAB>list"), ("PLA L1\n", "assign: line 1 of 'assign.txt' is not sample<TAB>list"),
          ("PLA\tL1\n\n", "assign: line 2 of 'assign.txt' is not sample<TAB>list"), ("PLA\tL1\textra\n", "assign: line 1 of 'assign.txt' is not sample<TAB>list"),
          ("\tL1\n", "assign: line 1 of 'assign.txt' is not sample<TAB>list"),
          ("PLA\tL1\nOTHER\tL1\n", "assign: line 2 names 'OTHER', which is no count file of S"),
          ("PLA\tL1\nPLA\tL9\n", "assign: line 2 names 'L9', which is no list of the variants file")]


def test_usage(tmp_path):
    for n in (0, 5, 11):
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


def test_the_two_lists(tmp_path):
    (tmp_path / "table.txt").write_text(TABLE)
    (tmp_path / "S").mkdir()
    (tmp_path / "S" / "PLA.PILEUP.ASEQ").write_text(HEADER)
    _refused(_run(EXE, TOKENS, tmp_path), f"{EXE} failed: variants: cannot read 'variants.txt'\n", tmp_path, "no variants")
    for text, answer in VARIANTS:
        (tmp_path / "variants.txt").write_text(text)
        _refused(_run(EXE, TOKENS, tmp_path), f"{EXE} failed: {answer}\n", tmp_path, text)
    (tmp_path / "variants.txt").write_text(GOOD)
    _refused(_run(EXE, TOKENS, tmp_path), f"{EXE} failed: assign: cannot read 'assign.txt'\n", tmp_path, "no assign")
    for text, answer in ASSIGN:
        (tmp_path / "assign.txt").write_text(text)
        _refused(_run(EXE, TOKENS, tmp_path), f"{EXE} failed: {answer}\n", tmp_path, text)
