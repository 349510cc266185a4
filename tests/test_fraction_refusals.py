"""What AmpliSolveTumourFraction refuses before it opens the device, as tests/test_monitor_refusals.py holds the monitoring command to it:
a wrong number of tokens (the usage text), every bad number, AMPLISOLVE_WORLD_SIZE=2, and every fault of the two lists: everything the
monitoring command refuses in them -- here with six columns --, plus a missing or bad weight.  The exit status is 1, stdout is exactly
the text below, stderr is empty and no output directory appears.  None of these runs reaches the device."""
from tests.test_cli_refusals import ORDER, _refused, _run
from tests.test_monitor_refusals import ASSIGN, HEADER, TABLE

EXE = "AmpliSolveTumourFraction"
TOKENS = ["errorFile=table.txt", "sample_dir=S", "variants=variants.txt", "assign=assign.txt", "coverage_cutoff=100", "min_variants=5", "max_vaf=1", "confidence=0.95",
          "output_dir=o"]
USAGE = ("Usage:\n\tAmpliSolveTumourFraction errorFile=<error table> sample_dir=<dir> variants=<file> assign=<file or -> coverage_cutoff=<int> "
         "min_variants=<int> max_vaf=<float> confidence=<0.90, 0.95 or 0.99> output_dir=<dir>" + ORDER +
         " (usual values: coverage_cutoff=100 min_variants=5 max_vaf=1 confidence=0.95).\n"
         "\tvariants: list<TAB>chrom<TAB>pos<TAB>ref<TAB>alt<TAB>weight per line, the weight in (0, 1]: the variant's allele fraction per unit "
         "of tumour fraction; assign: sample<TAB>list per line, or - for none; consecutive lines that name one list are consecutive draws.\n")
CONF = "confidence must be a number among 0.90, 0.95, 0.99, got "
BAD = [("coverage_cutoff", "-1", "coverage_cutoff must be an integer >= 0, got '-1'"), ("coverage_cutoff", "x", "coverage_cutoff must be an integer >= 0, got 'x'"),
       ("min_variants", "0", "min_variants must be an integer >= 1, got '0'"), ("min_variants", "2.5", "min_variants must be an integer >= 1, got '2.5'"),
       ("max_vaf", "1.5", "max_vaf must be a number in [0, 1], got '1.5'"), ("max_vaf", "-0.1", "max_vaf must be a number in [0, 1], got '-0.1'"),
       ("max_vaf", "x", "max_vaf must be a number in [0, 1], got 'x'"),
       ("confidence", "0.5", CONF + "'0.5'"), ("confidence", "0.975", CONF + "'0.975'"), ("confidence", "95", CONF + "'95'"), ("confidence", "", CONF + "''"),
       ("confidence", "nan", CONF + "'nan'"), ("confidence", "0.95x", CONF + "'0.95x'")]
SHAPE = " of 'variants.txt' is not list<TAB>chrom<TAB>pos<TAB>ref<TAB>alt<TAB>weight"
GOOD = "L1\tchr7\t100\tA\tC\t0.4\n"
WEIGHT = "variants: line 1: weight must be a number in (0, 1], got "
VARIANTS = [(GOOD + "L1\tchr7\t101\tG\tA\n", "variants: line 2" + SHAPE),  # the weight is missing: monitoring's five columns
            ("L1 chr7 100 A C 0.4\n", "variants: line 1" + SHAPE), (GOOD + "\n" + GOOD, "variants: line 2" + SHAPE),
            ("L1\tchr7\t100\tA\tC\t0.4\textra\n", "variants: line 1" + SHAPE), ("\tchr7\t100\tA\tC\t0.4\n", "variants: line 1" + SHAPE),
            ("L1\t\t100\tA\tC\t0.4\n", "variants: line 1" + SHAPE),
            ("L1\tchr7\t1e2\tA\tC\t0.4\n", "variants: line 1: pos must be a whole positive number, got '1e2'"),
            ("L1\tchr7\t0\tA\tC\t0.4\n", "variants: line 1: pos must be a whole positive number, got '0'"),
            ("L1\tchr7\t-100\tA\tC\t0.4\n", "variants: line 1: pos must be a whole positive number, got '-100'"),
            ("L1\tchr7\t\tA\tC\t0.4\n", "variants: line 1: pos must be a whole positive number, got ''"),
            ("L1\tchr7\t100\tA\tN\t0.4\n", "variants: line 1: ref and alt must each be one of A, C, G, T, got 'A' and 'N'"),
            ("L1\tchr7\t100\ta\tC\t0.4\n", "variants: line 1: ref and alt must each be one of A, C, G, T, got 'a' and 'C'"),
            ("L1\tchr7\t100\tA\tCT\t0.4\n", "variants: line 1: ref and alt must each be one of A, C, G, T, got 'A' and 'CT'"),
            ("L1\tchr7\t100\tA\tA\t0.4\n", "variants: line 1: alt equals ref ('A')"),
            ("L1\tchr7\t100\tA\tC\t\n", WEIGHT + "''"), ("L1\tchr7\t100\tA\tC\t0\n", WEIGHT + "'0'"), ("L1\tchr7\t100\tA\tC\t-0.2\n", WEIGHT + "'-0.2'"),
            ("L1\tchr7\t100\tA\tC\t1.0001\n", WEIGHT + "'1.0001'"), ("L1\tchr7\t100\tA\tC\tnan\n", WEIGHT + "'nan'"), ("L1\tchr7\t100\tA\tC\tinf\n", WEIGHT + "'inf'"),
            ("L1\tchr7\t100\tA\tC\t0.4x\n", WEIGHT + "'0.4x'"), ("L1\tchr7\t100\tA\tC\t40%\n", WEIGHT + "'40%'"), ("L1\tchr7\t100\tA\tC\t1e-60\n", WEIGHT + "'1e-60'"),
            (GOOD + "L1\tchr7\t102\tA\tC\t0.4\n", "variants: line 2: chr7:102 is not a position of the error table"),
            ("L1\tchr8\t100\tA\tC\t0.4\n", "variants: line 1: chr8:100 is not a position of the error table"),
            (GOOD + "L2\tchr7\t101\tA\tC\t1\n", "variants: line 2: ref 'A' is not the table's base 'G' at chr7:101"),
            ("", "variants: 'variants.txt' lists no variant")]


def test_usage(tmp_path):
    for n in (0, 5, 8):
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
