"""CPU: the committed edge cases of the pairing kernels (tests/golden/pairing_edges.json.gz, made by
tools/make_pairing_edges_golden.py from tests/pairing_edge_lib.py).  The oracle reproduces every case, the reference
every case it answered; the cases reach what each group is aimed at (the cover); and the fixture tells apart the changes
of input, and of the threshold rule, it is meant to notice."""
import os

import pytest

import oracle_lib as O
import pairing_edge_lib as E

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
needs_ref = pytest.mark.skipif(not O.have_ref(), reason="oracle/_ref not built")


@pytest.fixture(scope="module")
def fixture():
    return E.load_fixture(os.path.join(GOLD, "pairing_edges.json.gz"))


@pytest.fixture(scope="module")
def answers(fixture):
    """the oracle's pairings and locus depths of every case, computed once"""
    return {g: [E.oracle_answers(c[1], c[2], c[3], depths=True) for c, _, _ in fixture[g]] for g in E.GROUPS}


def test_fixture_holds_the_generators_cases(fixture):
    """the inputs in the file are the ones the seeded generators give today: the GPU tests' fresh seeds are others"""
    for g in E.GROUPS:
        want = E.cases(g)
        assert [c for c, _, _ in fixture[g]] == [(n, gen, ests, [tuple(p) for p in prm]) for n, gen, ests, prm in want], g


@pytest.mark.parametrize("group", E.GROUPS)
def test_oracle_reproduces_the_fixture(fixture, answers, group):
    n = 0
    for (c, stored, _), ans in zip(fixture[group], answers[group]):
        for (L, rate), per_est, want in zip(c[3], ans, stored):
            for k, ((tri, _), w) in enumerate(zip(per_est, want)):
                assert tri.tolist() == w, (c[0], L, rate, k)
                n += 1
    assert n >= len(fixture[group])


@needs_ref
@pytest.mark.parametrize("group", E.GROUPS)
def test_reference_reproduces_its_cases(fixture, group):
    """RefIndex preprocessed at the case's min_factor_len, in a child process (one per group)"""
    mine = [(c, stored) for c, stored, by in fixture[group] if by == "reference"]
    assert mine
    got = E.reference_answers([(c[1], c[2], c[3]) for c, _ in mine])
    assert got is not None, "the reference's process died"
    for (c, stored), g in zip(mine, got):
        assert g == stored, c[0]


def test_only_what_the_reference_cannot_answer_is_the_oracles_alone(fixture):
    for g in E.GROUPS:
        for c, _, by in fixture[g]:
            assert by in ("reference", "oracle")
            if by == "oracle":
                assert len(c[1]) < 64 or all(L in E.REFERENCE_DIES_AT_L for L, _ in c[3]), c[0]


def test_cover(fixture, answers):
    """Every group reaches its target, counted by the tag functions over the cases the reference answered (min_factor_len
    1, where it answers nothing, over the oracle's)."""
    tagged, lone = {}, {}
    for g in E.GROUPS:
        tagged[g] = [E.tags(g, c, a) for (c, _, by), a in zip(fixture[g], answers[g]) if by == "reference"]
        lone[g] = [E.tags(g, c, a) for (c, _, by), a in zip(fixture[g], answers[g]) if by != "reference"]
    counts, lacks = E.cover(tagged, lone)
    print(counts)
    assert not lacks, lacks
    n = {g: {} for g in E.GROUPS}
    for g in E.GROUPS:
        for ts in tagged[g]:
            for x in ts:
                n[g][x] = n[g].get(x, 0) + 1
    for L in E.SMALL_LS:
        assert ("L", L) in n["small_L"] or (L in E.REFERENCE_DIES_AT_L and any(("L", L) in ts for ts in lone["small_L"])), L
    for tr in E.RES:
        for ir in E.RES:
            for ln in E.LENS:
                assert n["windows"].get(("res", tr, ir, ln)), (tr, ir, ln)
    for b in E.FLAG_BYTES:
        assert n["flagged"].get(("gen", b)) and n["flagged"].get(("est", b)) and n["flagged"].get(("both", b)), chr(b)
    assert n["threshold"].get("truncation", 0) >= 3
    assert n["order"].get("repeated", 0) >= 20
    assert n["crowded"].get("list64", 0) >= 1 and n["crowded"].get("filter_b", 0) >= 1
    # the table of tests/golden/pairing_edges.md is this one
    md = open(os.path.join(GOLD, "pairing_edges.md")).read()
    for k, v in counts.items():
        assert "| %s | %s |" % (k, v) in md, k


def test_fixture_notices_what_it_is_aimed_at(fixture):
    seen = E.notices({g: [(c, stored) for c, stored, _ in fixture[g]] for g in E.GROUPS})
    print(seen)
    upper, masks, exact = seen.values()
    assert upper >= 10 and masks >= 10 and exact >= 3
    md = open(os.path.join(GOLD, "pairing_edges.md")).read()
    for k, v in seen.items():
        assert "| %s | %s |" % (k, v) in md, k


def test_thresholds_sit_on_the_doubles_truncation():
    """the products the `threshold` group is built on: below an integer in double, that integer as a rational"""
    for D, rate in E.THRESHOLDS:
        assert E.double_threshold(D, rate, 15) + 1 == E.exact_threshold(D, rate, 15), (D, rate)
    assert E.double_threshold(100, 0.29, 15) == 28 and E.double_threshold(60, 0.25, 15) == 15 == E.exact_threshold(60, 0.25, 15)
