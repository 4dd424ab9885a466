"""CPU: the list stage's rules (include/pintron_gpu.h: pgpu_index_factorization_lists) restated (tests/flists_lib.py) against
the fixture tests/golden/factorization_lists.json.gz, the fixture's cover and the conditions the GPU tests rest on, the wrong
rules it notices, the agreement with the factorization stage on every one-candidate case, the host code on records the fixture
does not hold, the binding's layout, and the host side of the entry under the sanitizers.  No GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cand_lib as KL
import enum_lib as EL
import fact_lib as FL
import flists_lib as F
import resource_lib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def restated():
    """the restatement's answer and info per fixture case, computed once"""
    seqs, cases, _ = F.load_fixture()
    out = []
    for c in cases:
        info = {}
        out.append((F.factorization_list(c["est"], seqs[c["seq"]], c["cands"], c["prm"], info), info))
    return out


def test_restatement_equals_the_fixture_on_every_case(restated):
    seqs, cases, _ = F.load_fixture()
    assert len(cases) > 800
    for c, (got, info) in zip(cases, restated):
        assert got == c["answer"], (c["seq"], c["name"])
        assert F.tags_of(got, info) == c["tags"], (c["seq"], c["name"])


def test_the_fixture_covers_every_tag_and_every_builder_reaches_its_tags():
    seqs, cases, _ = F.load_fixture()
    for t in F.TAGS:
        assert sum(1 for c in cases if t in c["tags"]) >= 1, t
    by_name = {c["name"]: c for c in cases}
    g, hand = F.hand_cases()
    for name, est, cands, prm, want in hand + F.cap_cases(g):
        c = by_name["hand/" + name]
        assert (c["est"], c["cands"], c["prm"]) == (est, [[tuple(e) for e in x] for x in cands], prm), name
        assert set(want) <= set(c["tags"]), (name, want, c["tags"])
    assert sum(1 for name, *_ in F.generated_cases(g) if "done_2_or_more" in by_name[name]["tags"]) >= 20
    assert by_name["hand/cands_64"]["answer"]["counts"] == (64, 64, 64) and len(by_name["hand/cands_64"]["answer"]["facts"]) == 64
    assert (by_name["hand/cands_65"]["answer"]["outcome"], by_name["hand/cands_65"]["answer"]["detail"]) == (F.HOST, F.CAP_CANDIDATES)
    # the widening is in the answer: head only, tail only, both
    for name, flags in (("widen_head", F.HEAD_WIDENED), ("widen_tail", F.TAIL_WIDENED), ("widen_both", F.HEAD_WIDENED | F.TAIL_WIDENED)):
        a, plain = by_name["hand/" + name]["answer"], by_name["hand/one_candidate"]["answer"]
        assert [f["flags"] for f in a["facts"]] == [flags] and a["facts"][0]["exons"] == plain["facts"][0]["exons"], name
    # the filtered entry never met the cap that makes it HOST when the filter is off
    assert by_name["hand/filtered_before_cap"]["answer"]["outcome"] == F.DONE
    assert (by_name["hand/gaps_cap_second"]["answer"]["outcome"], by_name["hand/gaps_cap_second"]["answer"]["stage"]) == (F.HOST, 3)


def test_the_conditions_the_gpu_tests_rest_on(restated):
    seqs, cases, counts = F.load_fixture()
    multi = [(c, a, info) for c, (a, info) in zip(cases, restated) if len(c["cands"]) >= 2]
    host = sum(1 for c, a, _ in multi if a["outcome"] == F.HOST)
    done2 = sum(1 for c, a, _ in multi if a["outcome"] == F.DONE and len(a["facts"]) >= 2)
    widened = sum(1 for c, a, info in multi if info.get("widened"))
    assert 5 * host <= len(multi), (host, len(multi))
    assert done2 >= 50, done2
    assert widened >= 20, widened
    assert (counts["multi"], counts["multi_host"], counts["multi_done_2"], counts["widened"]) == (len(multi), host, done2, widened)
    text = open(os.path.join(HERE, "golden", "factorization_lists.md")).read()
    assert "cases with two or more candidates: %d; of them HOST: %d, DONE with two or more factorizations: %d, with a -2 widening: %d" \
        % (len(multi), host, done2, widened) in text


@pytest.mark.parametrize("wrong", F.WRONG_RULES)
def test_the_fixture_notices_a_wrong_rule(wrong):
    seqs, cases, _ = F.load_fixture()
    noticed = 0
    for c in cases:
        if len(c["cands"]) < 2 or len(c["cands"]) > 12:
            continue
        if F.factorization_list(c["est"], seqs[c["seq"]], c["cands"], c["prm"], wrong=wrong) != c["answer"]:
            noticed += 1
            if noticed >= 2:
                break
    assert noticed >= 1, wrong


def test_one_candidate_cases_agree_with_the_factorization_stage(restated):
    seqs, cases, _ = F.load_fixture()
    n = 0
    for c, (a, _) in zip(cases, restated):
        if len(c["cands"]) != 1:
            continue
        f = FL.factorization(KL.ONE, c["est"], seqs[c["seq"]], c["cands"][0], c["prm"][:5])
        stage = {0: 0, 1: 1, 2: 3, 3: 4}[f["stage"]]
        assert (a["outcome"], a["stage"]) == (f["outcome"], stage), c["name"]
        if f["outcome"] == F.HOST:
            assert a["detail"] == f["detail"], c["name"]
        if f["outcome"] == F.DONE:
            (x,) = a["facts"]
            assert (x["exons"], x["steps"], x["n_merged"], x["total_edit"], x["flags"]) == \
                (f["exons"], f["steps"], f["n_merged"], f["total_edit"], f["detail"]), c["name"]
        n += 1
    assert n >= 70


def test_restatement_equals_the_host_code_on_records_the_fixture_does_not_hold():
    """the one-path records of candidate_lists.json.gz that the fixture's sample left out, and a second parameter set"""
    seqs, cases, _ = F.load_fixture()
    held = {c["name"] for c in cases}
    _, ecases, _ = EL.load_fixture()
    todo = [c for c in ecases if c["name"].startswith(("path/", "empty/")) and c["name"] not in held and F.real_case(c)]
    assert len(todo) > 200
    hosts, n = {}, 0
    try:
        for c in todo[::3]:
            est, cands, prm = F.real_case(c)
            for p in (prm, F.params(min_intron_length=c["min_intron"], max_coverage_diff=1.0, max_site_difference=3, max_gaplength_diff=-1)):
                a = F.factorization_list(est, seqs[c["seq"]], cands, p)
                if a["outcome"] == F.HOST:
                    continue
                if c["seq"] not in hosts:
                    hosts[c["seq"]] = F.Host(seqs[c["seq"]])
                assert F.agrees_with_host(a, hosts[c["seq"]].factorizations(c["record"], est, c["L"], p)), (c["name"], p)
                n += 1
    finally:
        for h in hosts.values():
            h.close()
    assert n > 100


def test_binding_matches_the_header():
    from pintron_amd import capi
    import binding_lib as B
    names = ["pgpu_index_factorization_lists", "pgpu_index_factorization_lists_kernel_ms", "pgpu_pairing_plan_run_factorization_lists",
             "pgpu_pairing_plan_factorization_list_counts", "pgpu_pairing_plan_fetch_factorization_lists",
             "pgpu_pairing_plan_factorization_lists_ms"]
    assert all(n in capi.EXPORTS for n in names)
    L = capi.lib()
    assert all(hasattr(L, n) for n in names) and L.pgpu_abi_version() == 1
    size_of = dict(B.SIZE_OF, uint16_t=2, uint8_t=1)
    for cname, struct_, dtype in (("pgpu_flist_params", capi.FlistParams, capi.FLIST_PARAMS_DTYPE),
                                  ("pgpu_flist_query", capi.FlistQuery, capi.FLIST_QUERY_DTYPE),
                                  ("pgpu_flist_result", capi.FlistResult, capi.FLIST_RESULT_DTYPE),
                                  ("pgpu_flist_fact", capi.FlistFact, capi.FLIST_FACT_DTYPE)):
        fields, size = B.header_struct(cname)
        assert [f for f, _ in fields] == [f for f, _ in struct_._fields_] == [f for f, _ in dtype], cname
        off, dt = 0, np.dtype(dtype)
        for f, ctype in fields:
            assert getattr(struct_, f).offset == off == dt.fields[f][1], (cname, f)
            assert getattr(struct_, f).size == size_of[ctype] == dt.fields[f][0].itemsize, (cname, f)
            off += size_of[ctype]
        assert off == size == C.sizeof(struct_) == dt.itemsize, cname
    text = open(os.path.join(ROOT, "include", "pintron_gpu.h")).read()
    for name, value in (("MAX_CANDIDATES", 64), ("CAP_CANDIDATES", 4), ("DROPPED_FIRST", 1), ("HEAD_WIDENED", 2), ("TAIL_WIDENED", 4)):
        assert re.search(r"#define PGPU_FLIST_%s\s+%du\b" % (name, value), text), name
        assert getattr(capi, "FLIST_" + name) == getattr(F, name) == value
    # the defaults of the binding are the host configuration's
    p = capi.flist_params()
    assert (p.complexity_threshold, p.suffpref_length_on_est, p.suffpref_length_for_intron, p.suffpref_length_on_gen, p.min_intron_length,
            p.max_coverage_diff, p.max_site_difference, p.max_gaplength_diff, p.max_number_of_factorizations) == F.DEFAULTS


def test_host_side_of_the_entry_under_sanitizers(tmp_path):
    hipcc = resource_lib.hipcc()
    if not hipcc:
        pytest.skip("no ROCm headers here")
    include = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "include")
    exe = str(tmp_path / "flists_call_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", "-I" + include, "-o", exe,
                    os.path.join(HERE, "hostcheck", "flists_call_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == "ok\n", (r.stdout, r.stderr[-2000:])
