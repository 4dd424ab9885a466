"""CPU: the candidate stage's restatement (tests/cand_lib.py) against the fixture whose Burset frequencies are the
reference's, the fixture's cover, the restatement against the host's ef_chain_candidate on graphs the fixture does not
hold, the binding against the header, and the host side of pgpu_index_candidates under the sanitizers."""
import ctypes as C
import os
import re
import subprocess

import pytest

import cand_lib as CL
import resource_lib

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_restatement_equals_the_fixture_on_every_case():
    seqs, cases = CL.load_fixture()
    for c in cases:
        info = {}
        got = CL.candidate(c["record"], seqs[c["seq"]], c["L"], c["min_intron"], info=info)
        assert got == (c["kind"], c["work"], c["n_pairs"], c["exons"]), (c["seq"], c["name"])
        assert CL.tags_of(info) == c["tags"], (c["seq"], c["name"])
        assert not any(k in info for k in CL.NEVER), (c["seq"], c["name"], info)
        assert not CL.record_einval(c["record"], len(seqs[c["seq"]])), (c["seq"], c["name"])


def test_the_fixture_covers_what_it_must():
    seqs, cases = CL.load_fixture()
    cov = CL.cover(cases)
    assert set(seqs) == {"hand", "c2", "ambn", "issue13"}
    assert all(n > 0 for n in cov["kinds"]), cov
    for t in CL.TAGS:                                          # every branch has a case ...
        assert cov["tags"][t] >= 1, t
    for t in ("refuse_deltas", "refuse_lengths", "refuse_diagonal", "empty_range", "tie"):      # ... these five each
        assert cov["tags"][t] >= 5, (t, cov["tags"][t])
    hand = {c["name"]: c for c in cases if c["seq"] == "hand"}
    assert set(CL.NOT_PATH_WAYS) <= set(hand) and all(hand[w]["kind"] == CL.NOT_PATH for w in CL.NOT_PATH_WAYS)
    assert hand["flag_unavailable"]["kind"] == hand["flag_too_complex"]["kind"] == hand["flag_both"]["kind"] == CL.NONE
    assert hand["source_sink_only"]["kind"] == CL.REFUSED and hand["source_sink_only"]["work"] == 2
    assert hand["vertices_64"]["kind"] == CL.ONE and hand["vertices_64"]["n_pairs"] == 62 and hand["vertices_64"]["work"] == 64 + 63
    assert hand["vertices_64_backwards"]["exons"] == hand["vertices_64"]["exons"]
    # the last of equal cuts wins: the tie cases cut at the end of their range
    for k in range(5):
        c = hand["tie_%d" % k]
        assert c["kind"] == CL.ONE and c["exons"][0][1] == 139, c          # the node keeps all of its 40 bases: cut = node.p + node.l
    # an empty range leaves best_cut = 0 and the arithmetic goes on: the head begins at EST position 0
    assert all(hand["empty_range_%d" % k]["exons"][1][0] == 0 for k in range(5))
    # the real graphs: every set of every input, and under the defaults what the issue counted on test-issue-13
    for src in ("c2", "ambn", "issue13"):
        for set_name, _ in CL.fixture_sets():
            assert any(c["seq"] == src and c["name"].startswith(set_name + "/") for c in cases), (src, set_name)
    d13 = [c for c in cases if c["seq"] == "issue13" and c["name"].startswith("defaults/")]
    assert len(d13) == 1891 and sum(c["kind"] == CL.ONE for c in d13) > 800
    # the counts of candidates.md are the file's
    md = open(CL.FIXTURE[:-len(".json.gz")] + ".md").read()
    assert md.startswith("# `candidates.json.gz`") and ("%d MEG records" % len(cases)) in md
    assert ("0 none (flagged): %d, 1 not a path: %d, 2 refused: %d, 3 one candidate: %d" % tuple(cov["kinds"])) in md
    for t in CL.TAGS:
        assert re.search(r"`%s`: %d\b" % (t, cov["tags"][t]), md), t


def test_restatement_equals_the_host_code_on_graphs_not_in_the_fixture():
    import meg_lib as M
    gfa, efa, exons = M.sweep_sources()["repeats"]
    n_one = n_scan = 0
    for set_name, prm in M.sweep_sets(exons):
        recs, genomic = CL.host_records(gfa, efa, prm)
        gen_c = C.create_string_buffer(genomic, len(genomic) + 2)
        for k, rec in enumerate(recs):
            info = {}
            mine = CL.candidate(rec, genomic, prm["min_factor_len"], prm["min_intron_length"], info=info)
            assert mine == CL.host_candidate(rec, gen_c, prm["min_factor_len"], prm["min_intron_length"]), (set_name, k)
            assert not any(t in info for t in CL.NEVER), (set_name, k)
            n_one += mine[0] == CL.ONE
            n_scan += info.get("scan", 0)
    assert n_one > 50 and n_scan > 20, (n_one, n_scan)
    # ... and the hand-made records, which no host graph gives
    g = CL.hand_sequence()
    gen_c = C.create_string_buffer(g, len(g) + 2)
    for name, rec, L, mi in CL.hand_cases():
        assert CL.candidate(rec, g, L, mi) == CL.host_candidate(rec, gen_c, L, mi), name


def test_the_rules_on_the_input_restated():
    g = CL.hand_sequence()
    good = CL.record(*CL.chain([(100, 2000, 40), (140, 2200, 40)]))
    assert not CL.record_einval(good, len(g))
    for cut in range(len(good)):
        assert CL.record_einval(good[:cut], len(g)) == (cut < 16 + 48 + 10 + 3), cut
    blob, first = CL.batch([good, CL.bare(CL.UNAVAILABLE), good])
    assert not CL.einval(blob, first, len(g), 15)
    assert CL.einval(blob, first, len(g), 0) and CL.einval(blob, first, len(g), (1 << 24) + 1) and not CL.einval(blob, first, len(g), 1 << 24)
    assert CL.einval(blob[:-12], first, len(g), 15)
    assert CL.einval(blob, [0, 2, len(good)], len(g), 15)
    assert CL.einval(blob, first, 2239, 15) and not CL.einval(blob, first, 2240, 15)


def test_binding_matches_the_header():
    from pintron_amd import capi
    names = ["pgpu_pairing_plan_run_candidates", "pgpu_pairing_plan_candidate_exons", "pgpu_pairing_plan_fetch_candidates",
             "pgpu_pairing_plan_candidates_ms", "pgpu_index_candidates", "pgpu_index_candidates_kernel_ms"]
    assert all(n in capi.EXPORTS for n in names)
    L = capi.lib()
    assert all(hasattr(L, n) for n in names) and L.pgpu_abi_version() == 1
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pintron_gpu.h")).read(), flags=re.S)
    assert sorted(capi.EXPORTS) == sorted(set(re.findall(r"\b(pgpu_[a-z_0-9]+)\s*\(", hdr)))
    CL.assert_layout("pgpu_cand_params", capi.CandParams, capi.CAND_PARAMS_DTYPE)
    CL.assert_layout("pgpu_cand_result", capi.CandResult, capi.CAND_RESULT_DTYPE)
    text = open(os.path.join(ROOT, "include", "pintron_gpu.h")).read()
    for k, name in enumerate(("NONE", "NOT_PATH", "REFUSED", "ONE")):
        assert re.search(r"#define PGPU_CAND_%s\s+%du\b" % (name, k), text) and getattr(capi, "CAND_" + name) == getattr(CL, name) == k
    assert (capi.MEG_TOO_COMPLEX, capi.MEG_UNAVAILABLE) == (CL.TOO_COMPLEX, CL.UNAVAILABLE) == (1, 2)


def test_host_side_of_the_entry_under_sanitizers(tmp_path):
    hipcc = resource_lib.hipcc()
    if not hipcc:
        pytest.skip("no ROCm headers here")
    include = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "include")
    exe = str(tmp_path / "cand_call_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", "-I" + include, "-o", exe,
                    os.path.join(HERE, "hostcheck", "cand_call_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == "ok\n", (r.stdout, r.stderr[-2000:])
