"""CPU: the enumeration stage's rules (include/pintron_gpu.h: pgpu_index_candidate_lists) restated (tests/enum_lib.py) against
the fixture tests/golden/candidate_lists.json.gz, the fixture's cover, the wrong rules it notices, the caps on the real
graphs, the agreement with the candidate stage on every one-path record, the binding's layout, and the host side of the
entry under the sanitizers.  No GPU."""
import os
import re
import subprocess

import pytest

import cand_lib as CL
import enum_lib as EL
import resource_lib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def restated():
    """the restatement's answer and tags per fixture case, computed once"""
    seqs, cases, _ = EL.load_fixture()
    out = []
    for c in cases:
        info = {}
        out.append((EL.candidate_lists(c["record"], seqs[c["seq"]], c["L"], c["min_intron"], info=info), info))
    return out


def test_restatement_equals_the_fixture_on_every_case(restated):
    seqs, cases, _ = EL.load_fixture()
    for c, (got, info) in zip(cases, restated):
        assert got == EL.answer_of(c), (c["seq"], c["name"])
        assert EL.tags_of(info) == c["tags"], (c["seq"], c["name"])
        assert not any(k in info for k in CL.NEVER), (c["seq"], c["name"], info)
        assert not CL.record_einval(c["record"], len(seqs[c["seq"]])), (c["seq"], c["name"])


def test_the_fixture_covers_what_it_must():
    seqs, cases, _ = EL.load_fixture()
    assert set(seqs) == {"hand", "c2", "ambn", "issue13"}
    for t in EL.TAGS:
        n = sum(1 for c in cases if t in c["tags"])
        assert n >= (1 if t in EL.ONCE else 3), (t, n)
    hand = {c["name"][len("hand/"):]: c for c in cases if c["name"].startswith("hand/")}
    for k in range(3):
        for t in EL.RELATION_TAGS:                             # each outcome's builder reaches its outcome
            assert t in hand["%s_%d" % (t, k)]["tags"], (t, k)
        assert "removal_then_append" in hand["equal_2_%d" % k]["tags"] and "removal_then_append" in hand["longer_2_%d" % k]["tags"]
        assert "stop_at_0" in hand["equal_0_%d" % k]["tags"] and "stop_at_0" in hand["shorter_0_%d" % k]["tags"]
        # five vertices entered once each, five embeddings returned (x: 1, v: 1, w: 1, the source: 2)
        d = hand["diamond_%d" % k]
        assert "diamond" in d["tags"] and d["kind"] == EL.LISTS and d["n_roots"] == 1 and len(d["cands"]) == 2 and d["work"] == 5 + 5
        s = hand["second_root_%d" % k]
        assert s["n_roots"] == 2 and [r for r, _, _ in s["cands"]] == [0, 3] and "second_root" in s["tags"]
        assert "leaf_not_sink" in hand["leaf_not_sink_%d" % k]["tags"] and len(hand["leaf_not_sink_%d" % k]["cands"]) == 2
        r = hand["root_without_candidate_%d" % k]
        assert r["kind"] == EL.LISTS and r["n_roots"] == 2 and [x for x, _, _ in r["cands"]] == [0]
        e = hand["empty_graph_%d" % k]
        assert e["n_roots"] == 2 and e["work"] == 2 and [len(ex) for _, _, ex in e["cands"]] == [1, 1]
        assert hand["flag_unavailable_%d" % k]["kind"] == hand["flag_too_complex_%d" % k]["kind"] == EL.NONE
        assert hand["vertices_64_%d" % k]["kind"] == EL.LISTS and len(hand["vertices_64_%d" % k]["cands"]) == 2
        assert hand["degree_32_%d" % k]["kind"] == EL.LISTS and len(hand["degree_32_%d" % k]["cands"]) == 32
    for name in ("cycle", "self_loop", "cycle_unreached"):
        assert EL.answer_of(hand[name]) == (EL.CYCLIC, 0, 0, 0, []), name
    assert EL.answer_of(hand["no_vertex"]) == (EL.LISTS, 0, 0, 0, [])
    assert hand["edge_into_a_leaf_source"]["kind"] == EL.LISTS


def test_the_cap_edges(restated):
    seqs, cases, _ = EL.load_fixture()
    by_name = {c["name"]: (c, info) for c, (_, info) in zip(cases, restated)}
    c, info = by_name["hand/list_64"]
    assert c["kind"] == EL.LISTS and info["peak"] == EL.MAX_LIST and len(c["cands"]) == 64
    assert by_name["hand/list_65"][0]["kind"] == EL.RANGE and by_name["hand/list_65"][0]["detail"] == EL.CAP_LIST
    assert EL.answer_of(by_name["hand/list_80"][0]) == (EL.RANGE, EL.CAP_LIST, 0, 0, [])
    c, info = by_name["hand/embeddings_512"]
    assert c["kind"] == EL.LISTS and info["created"] == EL.MAX_EMBEDDINGS and info["peak"] <= EL.MAX_LIST
    assert EL.answer_of(by_name["hand/embeddings_513"][0]) == (EL.RANGE, EL.CAP_EMBEDDINGS, 0, 0, [])
    assert EL.created_by(*EL.EMB_512) == 512 and EL.created_by(*EL.EMB_513) == 513


@pytest.mark.parametrize("wrong", EL.WRONG_RULES)
def test_the_fixture_notices_a_wrong_rule(wrong):
    seqs, cases, _ = EL.load_fixture()
    noticed = 0
    for c in cases:
        if c["kind"] != EL.LISTS or len(c["record"]) > 2000:          # (small records suffice, and keep this quick)
            continue
        if EL.candidate_lists(c["record"], seqs[c["seq"]], c["L"], c["min_intron"], wrong=wrong) != EL.answer_of(c):
            noticed += 1
            if noticed >= 3:
                break
    assert noticed >= 3, (wrong, noticed)


def test_the_caps_on_the_real_graphs(restated):
    seqs, cases, counts = EL.load_fixture()
    real = [(c, got) for c, (got, _) in zip(cases, restated) if c["name"].startswith("real/") and c["seq"] != "hand"]
    assert len(real) == 676                                    # with cand_lib's five hand-made ones: 681 (candidate_lists.md)
    refused = [got[:2] for c, got in real if got[0] == EL.RANGE]
    lists = sum(1 for c, got in real if got[0] == EL.LISTS)
    assert len(refused) <= 30 and lists >= 640
    assert len(refused) == 24 and all(r == (EL.RANGE, EL.CAP_LIST) for r in refused) and lists == 652     # pinned: candidate_lists.md
    assert counts == {"real": 681, "real_lists": 656, "real_cap_list": 24, "real_cap_embeddings": 0, "real_cyclic": 1,
                      "peak": 60, "created": 190}


def test_one_path_records_agree_with_the_candidate_stage():
    seqs, cand_cases = CL.load_fixture()
    n = 0
    for c in cand_cases:
        if c["kind"] not in (CL.REFUSED, CL.ONE):
            continue
        kind, detail, work, n_roots, cands = EL.candidate_lists(c["record"], seqs[c["seq"]], c["L"], c["min_intron"])
        assert (kind, detail, work, n_roots) == (EL.LISTS, 0, c["work"], 1), (c["seq"], c["name"])
        if c["kind"] == CL.ONE:
            assert cands == [(0, c["n_pairs"], c["exons"])], (c["seq"], c["name"])
        else:
            assert cands == [], (c["seq"], c["name"])
        n += 1
    assert n >= 3500


def test_restatement_equals_the_host_code_on_the_hand_made_records():
    import ctypes as C
    g = CL.hand_sequence()
    gen_c = C.create_string_buffer(g, len(g) + 2)
    for name, rec, L, mi in EL.hand_cases():
        mine = EL.candidate_lists(rec, g, L, mi)
        if mine[0] in (EL.NONE, EL.LISTS):
            assert EL.host_candidate_lists(rec, gen_c, L, mi) == mine, name


def test_binding_matches_the_header():
    from pintron_amd import capi
    names = ["pgpu_pairing_plan_run_candidate_lists", "pgpu_pairing_plan_candidate_list_counts",
             "pgpu_pairing_plan_fetch_candidate_lists", "pgpu_pairing_plan_candidate_lists_ms", "pgpu_index_candidate_lists",
             "pgpu_index_candidate_lists_kernel_ms"]
    assert all(n in capi.EXPORTS for n in names)
    L = capi.lib()
    assert all(hasattr(L, n) for n in names) and L.pgpu_abi_version() == 1
    CL.assert_layout("pgpu_enum_result", capi.EnumResult, capi.ENUM_RESULT_DTYPE)
    CL.assert_layout("pgpu_enum_candidate", capi.EnumCandidate, capi.ENUM_CANDIDATE_DTYPE)
    text = open(os.path.join(ROOT, "include", "pintron_gpu.h")).read()
    for k, name in enumerate(("NONE", "CYCLIC", "RANGE", "LISTS")):
        assert re.search(r"#define PGPU_ENUM_%s\s+%du\b" % (name, k), text), name
        assert getattr(capi, "ENUM_" + name) == getattr(EL, name) == k
    for name, value in (("CAP_LIST", 1), ("CAP_EMBEDDINGS", 2), ("MAX_LIST", 64), ("MAX_EMBEDDINGS", 512)):
        assert re.search(r"#define PGPU_ENUM_%s\s+%du\b" % (name, value), text), name
        assert getattr(capi, "ENUM_" + name) == getattr(EL, name) == value


def test_host_side_of_the_entry_under_sanitizers(tmp_path):
    hipcc = resource_lib.hipcc()
    if not hipcc:
        pytest.skip("no ROCm headers here")
    include = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "include")
    exe = str(tmp_path / "enum_call_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", "-I" + include, "-o", exe,
                    os.path.join(HERE, "hostcheck", "enum_call_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == "ok\n", (r.stdout, r.stderr[-2000:])
