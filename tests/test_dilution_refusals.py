"""What AmpliSolveInSilicoDilution refuses before it opens the device, as tests/test_cli_refusals.py holds the other command lines to it:
a wrong number of tokens (the usage text), every bad number -- replicates outside 1 .. 2^20 - 1 among them --, AMPLISOLVE_WORLD_SIZE=2,
and every fault of the list of mixtures: a file that cannot be read, a malformed or empty line, a bad number, a file diluted with
itself, an unknown name, an empty list.  The exit status is 1, stdout is exactly the text below, stderr is empty and no output
directory appears.  None of these runs reaches the device."""
from tests.test_cli_refusals import ORDER, _refused, _run

EXE = "AmpliSolveInSilicoDilution"
TOKENS = ["errorFile=table.txt", "sample_dir=S", "mixtures=mixtures.txt", "replicates=8", "seed=1", "coverage_cutoff=100", "confidence=0.95", "write_counts=0",
          "output_dir=o"]
USAGE = ("Usage:\n\tAmpliSolveInSilicoDilution errorFile=<error table> sample_dir=<dir> mixtures=<file> replicates=<int> seed=<int> "
         "coverage_cutoff=<int> confidence=<0.5 .. 0.99> write_counts=<0 or 1> output_dir=<dir>" + ORDER +
         " (usual values: replicates=8 seed=1 coverage_cutoff=100 confidence=0.95 write_counts=0; "
         "mixtures lists source<TAB>diluent<TAB>fraction[<TAB>scale] per line, diluent - for none).\n")
REPS = "replicates must be an integer in [1, 1048575], got "
BAD = [("replicates", "0", REPS + "'0'"), ("replicates", "-3", REPS + "'-3'"), ("replicates", "1048576", REPS + "'1048576'"), ("replicates", "", REPS + "''"),
       ("replicates", "8x", REPS + "'8x'"), ("replicates", "2.5", REPS + "'2.5'"),
       ("seed", "", "seed must be an unsigned 64-bit integer, got ''"), ("seed", "-1", "seed must be an unsigned 64-bit integer, got '-1'"),
       ("seed", "1e3", "seed must be an unsigned 64-bit integer, got '1e3'"),
       ("seed", "18446744073709551616", "seed must be an unsigned 64-bit integer, got '18446744073709551616'"),
       ("coverage_cutoff", "0", "coverage_cutoff must be an integer >= 1, got '0'"), ("coverage_cutoff", "x", "coverage_cutoff must be an integer >= 1, got 'x'"),
       ("confidence", "0.4", "confidence must be a number in [0.5, 0.99], got '0.4'"), ("confidence", "0.995", "confidence must be a number in [0.5, 0.99], got '0.995'"),
       ("confidence", "nan", "confidence must be a number in [0.5, 0.99], got 'nan'"), ("confidence", "", "confidence must be a number in [0.5, 0.99], got ''"),
       ("write_counts", "2", "write_counts must be an integer in [0, 1], got '2'"), ("write_counts", "yes", "write_counts must be an integer in [0, 1], got 'yes'")]
HEADER = "chr\tpos\tdbsnp\tMAF\tref\talt\tA\tC\tG\tT\tRD\tArs\tCrs\tGrs\tTrs\n"
SHAPE = " of 'mixtures.txt' is not source<TAB>diluent<TAB>fraction[<TAB>scale]"
LISTS = [("TUM\tNORM\t0.5\nTUM\tNORM\n", "mixtures: line 2" + SHAPE),
         ("TUM NORM 0.5\n", "mixtures: line 1" + SHAPE),
         ("TUM\tNORM\t0.5\t1\textra\n", "mixtures: line 1" + SHAPE),
         ("\tNORM\t0.5\n", "mixtures: line 1" + SHAPE),
         ("TUM\t\t0.5\n", "mixtures: line 1" + SHAPE),
         ("TUM\tNORM\t0.5\n\nTUM\t-\t0.1\n", "mixtures: line 2" + SHAPE),
         ("TUM\tNORM\t1.5\n", "mixtures: line 1: fraction must be a number in [0, 1], got '1.5'"),
         ("TUM\tNORM\t-0.1\n", "mixtures: line 1: fraction must be a number in [0, 1], got '-0.1'"),
         ("TUM\tNORM\t\n", "mixtures: line 1: fraction must be a number in [0, 1], got ''"),
         ("TUM\tNORM\t0.5x\n", "mixtures: line 1: fraction must be a number in [0, 1], got '0.5x'"),
         ("TUM\tNORM\tnan\n", "mixtures: line 1: fraction must be a number in [0, 1], got 'nan'"),
         ("TUM\tNORM\t0.5\t0\n", "mixtures: line 1: scale must be a number in (0, 1], got '0'"),
         ("TUM\tNORM\t0.5\t1.01\n", "mixtures: line 1: scale must be a number in (0, 1], got '1.01'"),
         ("TUM\tNORM\t0.5\t\n", "mixtures: line 1: scale must be a number in (0, 1], got ''"),
         ("TUM\tNORM\t0.5\nNORM\tNORM\t0.5\n", "mixtures: line 2 dilutes 'NORM' with itself"),
         ("TUM\tNORM\t0.5\nTUM\tOTHER\t0.5\n", "mixtures: line 2 names 'OTHER', which is no count file of S"),
         ("-\tNORM\t0.5\n", "mixtures: line 1 names '-', which is no count file of S"),
         ("tum\t-\t0.5\n", "mixtures: line 1 names 'tum', which is no count file of S"),
         ("", "mixtures: 'mixtures.txt' lists no mixture")]


def test_usage(tmp_path):
    for n in (0, 4, 8):
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


def test_the_list_of_mixtures(tmp_path):
    (tmp_path / "S").mkdir()
    for name in ("TUM", "NORM"):
        (tmp_path / "S" / f"{name}.PILEUP.ASEQ").write_text(HEADER)
    _refused(_run(EXE, TOKENS, tmp_path), f"{EXE} failed: mixtures: cannot read 'mixtures.txt'\n", tmp_path, "no list")
    for text, answer in LISTS:
        (tmp_path / "mixtures.txt").write_text(text)
        _refused(_run(EXE, TOKENS, tmp_path), f"{EXE} failed: {answer}\n", tmp_path, text)
