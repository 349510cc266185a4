"""ampli_host_phase_score, the host library's twin of ampli_phase_score (the same ampli_ph_* of csrc/ampli_math.h compiled for the host),
and the command's part behind the walk (ampli_host_phase_files: the pair builder, the verdicts, the chain builder, both writers) against
the model without a device: integers and classes exact, |score| within S_TOL, the two files byte for byte."""
import ctypes as C

import numpy as np
import pytest

from tests import phase_model as ph


host_score = ph.host_score


@pytest.mark.parametrize("name", [c[0] for c in ph.score_cases()])
def test_score_cases(name):
    _, table, cells, nts, min_alt, min_share = next(c for c in ph.score_cases() if c[0] == name)
    found = ph.score_differences(host_score(table, cells, nts, min_alt, min_share), ph.score(table, cells, nts, min_alt, min_share))
    assert not found, found


def test_random_tables():
    t, cells, nts = ph.random_tables(np.random.default_rng(3202), 60)
    for min_alt, min_share in ((4, 10), (1, 0), (20, 100)):
        found = ph.score_differences(host_score(t, cells, nts, min_alt, min_share), ph.score(t, cells, nts, min_alt, min_share))
        assert not found, found


def test_the_table_of_a_counted_stream():
    case = next(c for c in ph.cases() if c.name.endswith("_900_reads_dense"))
    t = case.want().table
    rng = np.random.default_rng(3203)
    cells = rng.integers(0, len(t) * ph.K, size=400)
    ref = rng.integers(0, 4, size=(400, 2))
    alt = (ref + 1 + rng.integers(0, 3, size=(400, 2))) % 4
    nts = np.stack([ref[:, 0], alt[:, 0], ref[:, 1], alt[:, 1]], 1)
    want = ph.score(t, cells, nts, 1, 0)  # (random bases: a handful of reads per corner)
    assert (want.cls > 0).sum() >= 20 and (want.score != 0).sum() >= 20
    found = ph.score_differences(host_score(t, cells, nts, 1, 0), want)
    assert not found, found


def test_arguments():
    from amplisolve_amd import host_lib

    lib = host_lib()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    keep = [np.zeros((2, ph.K, ph.PAIR), np.int32), np.zeros(1, np.int64), np.zeros(4, np.int8), np.zeros(6, np.int64), np.zeros(1, np.float32), np.zeros(1, np.int32)]
    good = [ptr(keep[0]), 2, ptr(keep[1]), ptr(keep[2]), 1, 4, 10, ptr(keep[3]), ptr(keep[4]), ptr(keep[5])]
    assert lib.ampli_host_phase_score(*good) == 0
    for at, bad in ((0, None), (1, -1), (2, None), (3, None), (4, -1), (5, 0), (6, -1), (6, 101), (7, None), (8, None), (9, None)):
        args = list(good)
        args[at] = bad
        assert lib.ampli_host_phase_score(*args) != 0, at
    assert lib.ampli_host_phase_score(*good[:4], 0, *good[5:]) == 0


def host_files(tmp_path, lines, index, table, p, name="S"):
    from amplisolve_amd import host_lib

    table = np.ascontiguousarray(table, np.int32)
    text = "".join(f"{c}\t{pos}\t{ref}\t{alt}\n" for c, pos, ref, alt in lines).encode()
    idx = np.asarray(index, np.int64)
    stats = np.zeros(3, np.int64)
    rc = host_lib().ampli_host_phase_files(text, idx.ctypes.data_as(C.c_void_p), len(lines), table.ctypes.data_as(C.c_void_p), len(table), p["min_alt"], p["min_share"],
                                           float(p["q_min"]), p["max_dist"], str(tmp_path).encode(), name.encode(), stats.ctypes.data_as(C.c_void_p))
    assert rc == 0, host_lib().ampli_host_last_error()
    return (tmp_path / f"{name}.PHASE.txt").read_text(), (tmp_path / f"{name}.PHASE.MNV.txt").read_text(), stats.tolist()


@pytest.mark.parametrize("name", [c.name for c in ph.cli_cases()])
def test_the_pair_and_chain_builders_and_both_writers_match_the_model(tmp_path, name):
    cli = next(c for c in ph.cli_cases() if c.name == name)
    keys, index = ph.cli_keys(cli)
    p = ph.cli_params(cli)
    table = ph.count(cli.reads, keys, p["mbq"], p["mrq"]).table
    got_ph, got_mnv, stats = host_files(tmp_path, cli.lines, index, table, p)
    want_ph, want_mnv = ph.files(cli.lines, index, table, p["min_alt"], p["min_share"], p["q_min"], p["max_dist"], scorer=host_score)
    assert got_ph == want_ph and got_mnv == want_mnv
    assert stats[0] == want_ph.count("\n") and stats[2] == want_mnv.count("\n")
    model_ph, model_mnv = ph.files(cli.lines, index, table, p["min_alt"], p["min_share"], p["q_min"], p["max_dist"])
    strip = lambda text: [line.split("\t")[:14] + line.split("\t")[15:] for line in text.splitlines()]  # noqa: E731  (all but the score's text)
    assert strip(got_ph) == strip(model_ph) and got_mnv == model_mnv
    assert sorted(x.name for x in tmp_path.iterdir()) == ["S.PHASE.MNV.txt", "S.PHASE.txt"]


def test_chains_of_three_and_lines_in_at_most_one_chain(tmp_path):
    """four consecutive positions all on the same reads: the first three make one chain, the fourth stays alone; and a table in which the
    middle pair is not CIS: two lines, no chain of three"""
    lines = [("chr1", 100 + i, "ACGT"[i % 4], "CGTA"[i % 4]) for i in range(4)]
    index = list(range(4))
    p = dict(min_alt=4, min_share=10, q_min=13.0, max_dist=200)
    t = np.zeros((4, ph.K, ph.STATES, ph.STATES), np.int64)
    for i in range(4):
        for j in range(i + 1, 4):
            ri, ai, rj, aj = i % 4, (i + 1) % 4, j % 4, (j + 1) % 4
            t[i, j - i - 1, ri, rj], t[i, j - i - 1, ai, aj] = 300, 30 + i + j
    got_ph, got_mnv, _ = host_files(tmp_path, lines, index, t, p)
    want_ph, want_mnv = ph.files(lines, index, t, **p)
    assert got_mnv == want_mnv == "chr1\t100\tACG\tCGT\t31\n" and [l.split("\t")[-1] for l in got_ph.splitlines()] == ["CIS"] * 6
    t[0, 1, 0, 2], t[0, 1, 1, 3], t[0, 1, 1, 2], t[0, 1, 0, 3] = 300, 0, 30, 30  # lines 0 and 2: TRANS
    got_ph, got_mnv, _ = host_files(tmp_path, lines, index, t, p, name="T")
    want_ph, want_mnv = ph.files(lines, index, t, **p)
    assert got_mnv == want_mnv == "chr1\t100\tAC\tCG\t31\nchr1\t102\tGT\tTA\t35\n"
    assert [l.split("\t")[:14] + l.split("\t")[15:] for l in got_ph.splitlines()] == [l.split("\t")[:14] + l.split("\t")[15:] for l in want_ph.splitlines()]


def test_a_directory_that_cannot_be_written_to_leaves_nothing(tmp_path):
    from amplisolve_amd import host_lib

    t = np.zeros((2, ph.K, ph.PAIR), np.int32)
    idx = np.asarray([0, 1], np.int64)
    rc = host_lib().ampli_host_phase_files(b"chr1\t5\tA\tC\nchr1\t6\tA\tC\n", idx.ctypes.data_as(C.c_void_p), 2, t.ctypes.data_as(C.c_void_p), 2, 4, 10, 13.0, 200,
                                           str(tmp_path / "missing").encode(), b"S", None)
    assert rc != 0 and b"cannot write" in host_lib().ampli_host_last_error() and list(tmp_path.iterdir()) == []
