"""The phasing model against itself (tests/phase_model.py; no GPU): the two restatements of the count agree on every case, every wrong
variant is caught by the deterministic cases named for it, the invariant ties the joint table to the counting model that is already
pinned (tests/pileup_model.py), and the planted pairs of the command's end-to-end case get the verdicts they were planted for."""
import numpy as np
import pytest

from tests import phase_model as ph

CASES = ph.cases()
BY_NAME = {c.name: c for c in CASES}


def test_the_constants_of_the_header_are_the_contracts():
    geo = ph.geometry()
    assert (geo.partners, geo.states, geo.other) == (ph.K, ph.STATES, ph.OTHER) == (8, 5, 4)
    assert geo.reads == 256 and 1 <= geo.window <= 256
    assert geo.window * geo.partners * geo.states * geo.states * 4 <= 64 * 1024  # the window's counters fit a workgroup's LDS


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_count_and_walk_agree(case):
    found = ph.differences(ph.walk(case.stream, case.keys, case.mbq, case.mrq), case.want())
    assert not found, found


@pytest.mark.parametrize("variant", sorted(ph.COUNT_VARIANTS))
def test_every_wrong_count_is_caught_by_its_named_cases(variant):
    assert set(ph.CAUGHT_BY) == set(ph.COUNT_VARIANTS)
    for name in ph.CAUGHT_BY[variant]:
        case = BY_NAME[name]
        assert ph.differences(case.want(wrong=variant), case.want()), f"{variant} ({ph.COUNT_VARIANTS[variant]}) goes unnoticed on {name}"


@pytest.mark.parametrize("variant", sorted(ph.SCORE_VARIANTS))
def test_every_wrong_score_is_caught_by_its_named_cases(variant):
    assert set(ph.SCORE_CAUGHT_BY) == set(ph.SCORE_VARIANTS)
    by_name = {c[0]: c[1:] for c in ph.score_cases()}
    for name in ph.SCORE_CAUGHT_BY[variant]:
        assert ph.score_differences(ph.score(*by_name[name], wrong=variant), ph.score(*by_name[name])), f"{variant} goes unnoticed on {name}"


invariant_failures = ph.invariant_failures


@pytest.mark.parametrize("name", sorted(ph.INVARIANT_CASES))
def test_the_invariant_holds_against_the_counting_model(name):
    case = BY_NAME[name]
    assert len(case.invariant_cells()) >= ph.INVARIANT_CASES[name]  # the precondition: both keys covered by the same kept reads
    bad = invariant_failures(case, case.want().table)
    assert not bad, bad[:3]


def test_the_invariant_sees_a_transposed_table():
    case = BY_NAME["leading_5S"]
    assert invariant_failures(case, case.want(wrong="table_transposed").table)


def test_the_planted_pairs_get_their_verdicts_and_no_score_sits_at_q_min():
    for cli in ph.cli_cases():
        keys, index = ph.cli_keys(cli)
        p = ph.cli_params(cli)
        table = ph.count(cli.reads, keys, p["mbq"], p["mrq"]).table
        ph_txt, mnv, rows = ph.files(cli.lines, index, table, p["min_alt"], p["min_share"], p["q_min"], p["max_dist"], rows=True)
        assert all(x is None or abs(abs(x) - p["q_min"]) > 2e-5 for _, _, _, x in rows), cli.name  # the verdicts are exact
        got = {(cli.lines[a][1], cli.lines[b][1]): v for a, b, v, _ in rows}
        for pair, v in cli.expect.items():
            assert got[pair] == v, (cli.name, pair, got[pair])
        assert ph_txt.count("\n") == len(rows)
        if cli.name == "planted_pairs":
            assert mnv == "chr1\t1010\tAA\tCC\t40\n" and len(rows) == 36
        if cli.name.startswith("a_pair_beyond_K"):
            assert sum(v == "NOT_FORMED" for _, _, v, _ in rows) == 2 and all(cli.lines[b][1] - cli.lines[a][1] <= 48 for a, b, _, _ in rows)
        if cli.name.startswith("an_unknown"):
            assert not any("chrUn" in line for line in ph_txt.splitlines()) and sum(v == "UNTESTED" for _, _, v, _ in rows) >= 3
        if cli.name.startswith("a_position_listed_twice"):
            assert len(rows) == 4 and mnv == "chr1\t1010\tAA\tCC\t40\n"


def test_random_tables_hold_enough_of_everything():
    t, cells, nts = ph.random_tables(np.random.default_rng(3201), 60)
    s = ph.score(t, cells, nts)
    assert (s.cls < 0).sum() >= 40 and all((s.cls == c).sum() >= 3 for c in range(8)) and (s.score > 13).sum() >= 10 and (s.score < -13).sum() >= 10
