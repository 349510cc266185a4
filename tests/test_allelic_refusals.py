"""What AmpliSolveAllelicImbalance refuses before it opens the device, as tests/test_cli_refusals.py holds the other command lines to it:
a wrong number of tokens (the usage text), every bad number, AMPLISOLVE_WORLD_SIZE=2, and every fault of `pairs` -- a file that cannot
be read, a malformed line, a tumour named twice, an unknown tumour, an unknown normal.  The exit status is 1, stdout is exactly the text
below, stderr is empty and no output directory appears.  None of these runs reaches the device."""
from tests.test_cli_refusals import ORDER, _refused, _run

EXE = "AmpliSolveAllelicImbalance"
TOKENS = ["panel_design=p.bed", "germline_dir=N", "tumour_dir=T", "pairs=self", "output_dir=o", "min_depth=100", "min_normals=5", "site_q=20", "min_sites=3",
          "q_min=20", "min_imbalance=0.02"]
USAGE = ("Usage:\n\tAmpliSolveAllelicImbalance panel_design=<bed> germline_dir=<dir> tumour_dir=<dir or -> pairs=<file or self> output_dir=<dir> "
         "min_depth=<int> min_normals=<int> site_q=<float> min_sites=<int> q_min=<float> min_imbalance=<float>" + ORDER +
         " (usual values: min_depth=100 min_normals=5 site_q=20 min_sites=3 q_min=20 min_imbalance=0.02).\n"
         "\ttumour_dir=-: the normals again (the null calibration); pairs: tumourName<TAB>normalName per line, or self.\n")
BAD = [("min_depth", "0", "min_depth must be an integer >= 1, got '0'"),
       ("min_depth", "", "min_depth must be an integer >= 1, got ''"),
       ("min_depth", "1e2", "min_depth must be an integer >= 1, got '1e2'"),
       ("min_normals", "0", "min_normals must be an integer >= 1, got '0'"),
       ("min_normals", "2.5", "min_normals must be an integer >= 1, got '2.5'"),
       ("site_q", "-1", "site_q must be a number in [0, 100], got '-1'"),
       ("site_q", "100.5", "site_q must be a number in [0, 100], got '100.5'"),
       ("site_q", "nan", "site_q must be a number in [0, 100], got 'nan'"),
       ("min_sites", "0", "min_sites must be an integer >= 1, got '0'"),
       ("min_sites", "x", "min_sites must be an integer >= 1, got 'x'"),
       ("q_min", "-5", "q_min must be a number in [0, 300], got '-5'"),
       ("q_min", "301", "q_min must be a number in [0, 300], got '301'"),
       ("q_min", "20q", "q_min must be a number in [0, 300], got '20q'"),
       ("min_imbalance", "-0.1", "min_imbalance must be a number in [0, 1], got '-0.1'"),
       ("min_imbalance", "1.5", "min_imbalance must be a number in [0, 1], got '1.5'"),
       ("min_imbalance", "inf", "min_imbalance must be a number in [0, 1], got 'inf'"),
       ("pairs", "", "pairs must be a file or self, got ''")]
HEADER = "chr\tpos\tdbsnp\tMAF\tref\talt\tA\tC\tG\tT\tRD\tArs\tCrs\tGrs\tTrs\n"
LISTS = [("TUM\tNORM\nFOLLOW\n", "pairs line 2 must be tumourName<TAB>normalName, got 'FOLLOW'"),
         ("TUM NORM\n", "pairs line 1 must be tumourName<TAB>normalName, got 'TUM NORM'"),
         ("TUM\tNORM\tOTHER\n", "pairs line 1 must be tumourName<TAB>normalName, got 'TUM\tNORM\tOTHER'"),
         ("\tNORM\n", "pairs line 1 must be tumourName<TAB>normalName, got '\tNORM'"),
         ("TUM\t\n", "pairs line 1 must be tumourName<TAB>normalName, got 'TUM\t'"),
         ("TUM\tNORM\n\nTUM\tOTHER\n", "pairs line 3 names TUM a second time"),
         ("tum\tNORM\n", "pairs names 'tum', which is no count file of T"),
         ("TUM.PILEUP.ASEQ\tNORM\n", "pairs names 'TUM.PILEUP.ASEQ', which is no count file of T"),
         ("TUM\tFOLLOW\n", "pairs names the normal 'FOLLOW', which is no count file of N"),
         ("NORM\tNORM\n", "pairs names 'NORM', which is no count file of T")]


def test_usage(tmp_path):
    for n in (0, 4, 10):
        _refused(_run(EXE, TOKENS[:n], tmp_path), USAGE, tmp_path, n)
    _refused(_run(EXE, TOKENS + ["extra=1"], tmp_path), USAGE, tmp_path, "one token too many")


def test_every_bad_value(tmp_path):
    for key, bad, answer in BAD:
        t = [f"{key}={bad}" if x.startswith(key + "=") else x for x in TOKENS]
        assert t != TOKENS
        _refused(_run(EXE, t, tmp_path), f"{EXE} failed: {answer}\n", tmp_path, (key, bad))


def test_one_gpu(tmp_path):
    _refused(_run(EXE, TOKENS, tmp_path, AMPLISOLVE_WORLD_SIZE="2"), f"{EXE} failed: {EXE} runs on one GPU: AMPLISOLVE_WORLD_SIZE > 1 is not supported\n",
             tmp_path, "AMPLISOLVE_WORLD_SIZE=2")


def test_pairs(tmp_path):
    for sub, names in (("N", ("NORM", "OTHER")), ("T", ("TUM", "FOLLOW"))):
        (tmp_path / sub).mkdir()
        for name in names:
            (tmp_path / sub / f"{name}.PILEUP.ASEQ").write_text(HEADER)
    tokens = [x if not x.startswith("pairs=") else "pairs=pairs.txt" for x in TOKENS]
    _refused(_run(EXE, tokens, tmp_path), f"{EXE} failed: cannot read pairs file pairs.txt\n", tmp_path, "no file")
    for text, answer in LISTS:
        (tmp_path / "pairs.txt").write_text(text)
        _refused(_run(EXE, tokens, tmp_path), f"{EXE} failed: {answer}\n", tmp_path, text)
    # with tumour_dir=- the files of pass 2 are the normals
    (tmp_path / "pairs.txt").write_text("TUM\tNORM\n")
    t = [x if not x.startswith("tumour_dir=") else "tumour_dir=-" for x in tokens]
    _refused(_run(EXE, t, tmp_path), f"{EXE} failed: pairs names 'TUM', which is no count file of N\n", tmp_path, "the normals again")
