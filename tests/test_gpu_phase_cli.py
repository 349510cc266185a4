"""computePhasing on the GPU (BAM + a list of calls -> .PHASE.txt + .PHASE.MNV.txt; ampli_pileup_phase over computeCounts' batch loop, then
one ampli_phase_score over the formed pairs) against the model of tests/phase_model.py on the same synthetic BAM files, byte for byte:
the planted pairs of one amplicon end to end, a position listed twice with two alts, an unknown chromosome, a multi-base alt, a pair
beyond K keys; an empty, a corrupt and a truncated file.

The text of a score is the one place where the device and the model may differ (the exact test runs through two math libraries: S_TOL),
so the expected files take their scores from the host library's twin of the kernel, which tests/test_phase_host.py holds to the model
within S_TOL; the model's own files must agree in every other column, and its verdicts are exact: no score of any case lies within 2e-5
of q_min (asserted on the model before the device is touched)."""
import os
import subprocess

import numpy as np
import pytest

from tests import helpers
from tests import phase_model as ph

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "amplisolve_amd", "bin")
REFS = [("chr1", 100000), ("chr8", 50000)]


def write_vcf(path, lines):
    with open(path, "w") as f:
        f.write("#chr\tpos\tid\tref\talt\n")
        for c, p, ref, alt in lines:
            f.write(f"{c}\t{p}\t.\t{ref}\t{alt}\n")


def run_ph(*args, env=None, **kw):
    return subprocess.run([f"{BIN}/computePhasing", *[str(a) for a in args]], capture_output=True, text=True, timeout=300,
                          env=dict(os.environ, AMPLISOLVE_STRICT_EXIT="1", **(env or {})), **kw)


def strip_score(text):
    return [line.split("\t")[:14] + line.split("\t")[15:] for line in text.splitlines()]


@pytest.mark.parametrize("name", [c.name for c in ph.cli_cases()])
def test_the_files_equal_the_model_byte_for_byte(tmp_path, name):
    cli = next(c for c in ph.cli_cases() if c.name == name)
    keys, index = ph.cli_keys(cli)
    p = ph.cli_params(cli)
    # ---- the model, before the device is touched ----
    res = ph.count(cli.reads, keys, p["mbq"], p["mrq"])
    args = (cli.lines, index, res.table, p["min_alt"], p["min_share"], p["q_min"], p["max_dist"])
    model_ph, model_mnv, rows = ph.files(*args, rows=True)
    assert all(x is None or abs(abs(x) - p["q_min"]) > 2e-5 for _, _, _, x in rows)  # no score in the band around q_min: the verdicts are exact
    got = {(cli.lines[a][1], cli.lines[b][1]): v for a, b, v, _ in rows}
    assert all(got[pair] == v for pair, v in cli.expect.items()), got
    want_ph, want_mnv = ph.files(*args, scorer=ph.host_score)
    assert strip_score(want_ph) == strip_score(model_ph) and want_mnv == model_mnv
    # ---- the command ----
    helpers.write_bam(tmp_path / "S1.bam", REFS, cli.reads, rng=np.random.default_rng(32), max_block=20000)
    write_vcf(tmp_path / "v.txt", cli.lines)
    out = tmp_path / "out"
    out.mkdir()
    tokens = [f"{k}={p[k]:g}" if k == "q_min" else f"{k}={p[k]}" for k in ("mbq", "mrq", "min_alt", "min_share", "q_min", "max_dist")]
    r = run_ph(f"vcf={tmp_path}/v.txt", f"bam={tmp_path}/S1.bam", "threads=3", *tokens, f"out={out}",
               env={"AMPLISOLVE_BAM_BATCH_BYTES": "70000"})  # many small batches: records and even the header span batch boundaries
    assert r.returncode == 0, r.stdout + r.stderr
    assert (out / "S1.PHASE.txt").read_text() == want_ph
    assert (out / "S1.PHASE.MNV.txt").read_text() == want_mnv
    assert sorted(os.listdir(out)) == ["S1.PHASE.MNV.txt", "S1.PHASE.txt"]  # no temporary file stays
    assert (f"{len(cli.reads)} alignment records (0 malformed), {res.stats[0]} kept (mrq {p['mrq']}), {res.stats[1]} over two or more of {len(cli.lines)} listed lines, "
            f"{res.stats[2]} cells counted (mbq {p['mbq']})") in r.stdout


def test_an_empty_a_corrupt_and_a_truncated_file(tmp_path):
    rng = np.random.default_rng(33)
    cli = ph.cli_cases()[0]
    keys, index = ph.cli_keys(cli)
    write_vcf(tmp_path / "v.txt", cli.lines)
    helpers.write_bam(tmp_path / "E.bam", REFS, [])
    (tmp_path / "e").mkdir()
    r = run_ph(f"vcf={tmp_path}/v.txt", f"bam={tmp_path}/E.bam", f"out={tmp_path}/e")
    assert r.returncode == 0, r.stdout + r.stderr
    want_ph, want_mnv = ph.files(cli.lines, index, np.zeros((len(keys), ph.K, ph.STATES, ph.STATES), np.int64))
    text = (tmp_path / "e" / "E.PHASE.txt").read_text()
    assert text == want_ph and len(text.splitlines()) == 36 and all(l.endswith("\t0\t0\t0\t0\t0\t0\t.\t0.0000\tUNTESTED") for l in text.splitlines())
    assert (tmp_path / "e" / "E.PHASE.MNV.txt").read_text() == want_mnv == ""
    assert sorted(os.listdir(tmp_path / "e")) == ["E.PHASE.MNV.txt", "E.PHASE.txt"]
    reads = helpers.random_amplicon_reads(rng, REFS, [(0, 1000, 1120), (1, 5000, 5100)], 800)
    helpers.write_bam(tmp_path / "C.bam", REFS, reads, rng=rng, max_block=5000, corrupt_block_size=(400, 0x7FFFFFFF))
    (tmp_path / "o").mkdir()
    r = run_ph(f"vcf={tmp_path}/v.txt", f"bam={tmp_path}/C.bam", f"out={tmp_path}/o")
    assert r.returncode != 0 and "computePhasing: " in r.stdout and "corrupt BAM record at uncompressed byte" in r.stdout
    assert os.listdir(tmp_path / "o") == []
    helpers.write_bam(tmp_path / "T.bam", REFS, reads[:50])  # a file cut off inside a record
    raw = (tmp_path / "T.bam").read_bytes()
    (tmp_path / "T.bam").write_bytes(raw[:len(raw) // 2])
    r = run_ph(f"vcf={tmp_path}/v.txt", f"bam={tmp_path}/T.bam", f"out={tmp_path}/o")
    assert r.returncode != 0 and os.listdir(tmp_path / "o") == []
