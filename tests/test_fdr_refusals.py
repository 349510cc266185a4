"""What AmpliSolveFalseDiscovery refuses before it opens the device, as tests/test_cli_refusals.py holds the other command lines to it: a
wrong number of tokens (the usage text), every bad value, an empty tumour directory and AMPLISOLVE_WORLD_SIZE=2.  The exit status is 1,
stdout is exactly the text below, stderr is empty and no output directory appears.  None of these runs reaches the device."""
from tests.test_cli_refusals import ORDER, _refused, _run

EXE = "AmpliSolveFalseDiscovery"
TOKENS = ["panel_design=p.bed", "reference_genome=unused.fa", "germline_dir=N", "tumour_dir=T", "C_value=0.002", "coverage_cutoff=100", "calling_cutoff=100",
          "fdr=0.05", "q_min=13", "output_dir=o"]
USAGE = ("Usage:\n\tAmpliSolveFalseDiscovery panel_design=<bed> reference_genome=<fasta> germline_dir=<dir> tumour_dir=<dir> C_value=<float> "
         "coverage_cutoff=<int> calling_cutoff=<int> fdr=<float> q_min=<float> output_dir=<dir>" + ORDER +
         " (usual values: C_value=0.002 coverage_cutoff=100 calling_cutoff=100 fdr=0.05 q_min=13).\n")
BAD = [("C_value", "", "C_value must be a number in [0, 1], got ''"),
       ("C_value", "1.5", "C_value must be a number in [0, 1], got '1.5'"),
       ("C_value", "0.002x", "C_value must be a number in [0, 1], got '0.002x'"),
       ("coverage_cutoff", "0", "coverage_cutoff must be an integer >= 1, got '0'"),
       ("coverage_cutoff", "2.5", "coverage_cutoff must be an integer >= 1, got '2.5'"),
       ("calling_cutoff", "-1", "calling_cutoff must be an integer >= 0, got '-1'"),
       ("fdr", "0", "fdr must be a number in (0, 1), got '0'"),
       ("fdr", "1", "fdr must be a number in (0, 1), got '1'"),
       ("fdr", "-0.05", "fdr must be a number in (0, 1), got '-0.05'"),
       ("fdr", "1.5", "fdr must be a number in (0, 1), got '1.5'"),
       ("fdr", "", "fdr must be a number in (0, 1), got ''"),
       ("fdr", "0.05x", "fdr must be a number in (0, 1), got '0.05x'"),
       ("fdr", "nan", "fdr must be a number in (0, 1), got 'nan'"),
       ("fdr", "inf", "fdr must be a number in (0, 1), got 'inf'"),
       ("q_min", "0", "q_min must be a number in (0, 100], got '0'"),
       ("q_min", "-5", "q_min must be a number in (0, 100], got '-5'"),
       ("q_min", "100.5", "q_min must be a number in (0, 100], got '100.5'"),
       ("q_min", "", "q_min must be a number in (0, 100], got ''"),
       ("q_min", "13q", "q_min must be a number in (0, 100], got '13q'")]


def test_usage(tmp_path):
    for n in (0, 4, 9):
        _refused(_run(EXE, TOKENS[:n], tmp_path), USAGE, tmp_path, n)
    _refused(_run(EXE, TOKENS + ["extra=1"], tmp_path), USAGE, tmp_path, "one token too many")


def test_every_bad_value(tmp_path):
    (tmp_path / "T").mkdir()
    (tmp_path / "T" / "X.PILEUP.ASEQ").write_text("")
    for key, bad, answer in BAD:
        t = [f"{key}={bad}" if x.startswith(key + "=") else x for x in TOKENS]
        assert t != TOKENS
        _refused(_run(EXE, t, tmp_path), f"{EXE} failed: {answer}\n", tmp_path, (key, bad))


def test_an_empty_tumour_directory(tmp_path):
    (tmp_path / "T").mkdir()
    _refused(_run(EXE, TOKENS, tmp_path), f"{EXE} failed: no *.ASEQ files in T\n", tmp_path, "an empty tumour directory")
    _refused(_run(EXE, [x.replace("tumour_dir=T", "tumour_dir=none") for x in TOKENS], tmp_path), f"{EXE} failed: no *.ASEQ files in none\n", tmp_path,
             "no tumour directory")


def test_one_gpu(tmp_path):
    _refused(_run(EXE, TOKENS, tmp_path, AMPLISOLVE_WORLD_SIZE="2"), f"{EXE} failed: {EXE} runs on one GPU: AMPLISOLVE_WORLD_SIZE > 1 is not supported\n",
             tmp_path, "AMPLISOLVE_WORLD_SIZE=2")
