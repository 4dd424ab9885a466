"""CPU: the final stage's restatement (tests/final_lib.py) against the host's own routines ef_chain_factorization ->
ef_chain_tail -> ef_chain_small on real inputs, the cover of what the GPU tests use, that those cases notice three wrong
ways to glue the stages, that the two trivial queries ask nothing, the binding against the header, and the host side of the
entries that makes no HIP call in a stand-alone program under AddressSanitizer and UBSan.

The cover, in cases of the hand-made groups (final_lib.hand_groups): every tag of final_lib.TAGS that is not in
final_lib.NOT_REACHED has at least MIN_PER_TAG = 3 cases that arrive through the stages.  The nine tags of NOT_REACHED cannot
arrive that way, for the reasons written beside that tuple; each has three cases among final_lib.probe_cases, stage results
made by hand that the GPU test sends through the hand-off kernels alone."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import cand_lib as KL
import fact_lib as F
import final_lib as FL
import small_lib as SL
import tail_lib as TL
import test_fact_cpu as TF

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.mark.parametrize("source", ["c2", "ambn", "issue13"])
def test_restatement_equals_the_host_code_on_real_inputs(source):
    """every one-path record: the candidate through the restatement, the record through the host's three routines, at the
    default settings and with min_intron_length 4 for the small stage"""
    genomic, rows = TF.real_answers(source)
    host, ops = SL.Host(genomic), SL.OracleOps(genomic)
    try:
        n_done = n_capped = n_one = 0
        for k, (rec, est, cand, _, _) in enumerate(rows):
            if cand[0] not in (KL.ONE, KL.REFUSED):
                continue
            n_one += 1
            host._set_mil(int(F.DEFAULTS[4]))
            kind, exons = host.factorization(rec, est)
            tail = host.tail(est, est, exons) if kind == 2 else None
            for mil in (int(F.DEFAULTS[4]), 4):
                info = {}
                mine = FL.final(cand[0], est, est, genomic, cand[3], F.DEFAULTS, mil, ops=ops, info=info)
                if mine["outcome"] == FL.HOST:                     # a cap of the device: the host has none
                    n_capped += 1
                    continue
                if mine["stage"] <= 3:
                    assert mine["outcome"] == FL.EMPTY and kind == 1, (source, k, kind, mine)
                    continue
                assert kind == 2, (source, k, kind, mine)
                dropped, polyA, polyadenil, left = tail
                assert (polyA, polyadenil) == (mine["polyA"], mine["polyadenil"]), (source, k)
                if (mine["outcome"], mine["stage"]) == (FL.EMPTY, 4):
                    assert dropped == 1, (source, k)
                    continue
                assert dropped == 0 and left == TL.kept_exons(info["tail_answer"]), (source, k, left)
                if info["small"].get("outside"):                   # the reference reads outside its strings there
                    continue
                emptied, final = host.small(est, est, left, mil)
                if mine["outcome"] == FL.EMPTY:
                    assert emptied == 1, (source, k, mil)
                else:
                    assert emptied == 0 and final == [tuple(e) for e in mine["exons"]], (source, k, mil, final, mine["exons"])
                    n_done += 1
        assert n_done > (n_one // 2 if source != "ambn" else 5), (n_done, n_one, n_capped)
    finally:
        host.close()


def test_the_cover_of_what_the_gpu_tests_use():
    count = {t: 0 for t in FL.TAGS}
    cells = set()
    n = 0
    for name, g, cases in FL.hand_groups():
        for c in cases:
            n += 1
            a = c["answer"]
            cells.add((a["outcome"], a["stage"], a["detail"]))
            assert c["tags"] <= set(FL.TAGS)
            for t in c["tags"]:
                count[t] += 1
    assert 100 <= n <= 600, n                                       # a GPU test over them stays within seconds
    for t in FL.TAGS:
        if t not in FL.NOT_REACHED:
            assert count[t] >= FL.MIN_PER_TAG, (t, count)
    # what cannot arrive through the stages 0-3 is run through the hand-off kernels over made-up stage results
    probes = FL.probe_cases()
    for t in FL.NOT_REACHED:
        assert sum(t in c["tags"] for c in probes) >= FL.MIN_PER_TAG, t
    (res, _, _), _ = FL.probe_expect(probes)
    reached = {(int(r["outcome"]), int(r["stage"]), int(r["detail"])) for r in res}
    assert {(FL.HOST, 4, 1), (FL.HOST, 4, 2), (FL.EMPTY, 4, 1), (FL.HOST, 5, 1), (FL.HOST, 5, 2), (FL.EMPTY, 5, 1), (FL.EMPTY, 5, 2),
            (FL.DONE, 5, 0), (FL.DONE, 5, 1)} <= reached
    assert {int(r["refused"]) for r in res} == {0, 1, 2, 3, 4, 5}
    assert any(r["outcome"] == FL.EMPTY and r["stage"] == 4 and r["polyA"] and r["polyadenil"] and r["tail_added"] for r in res)
    assert {(FL.DONE, 5, 0), (FL.HOST, 4, 1), (FL.HOST, 5, 1), (FL.EMPTY, 5, 1), (FL.EMPTY, 5, 2)} <= cells
    # the cells of the stages 0-3 come with the factorization stage's own hand-made cases
    assert {(FL.HOST, 0, KL.NONE), (FL.HOST, 1, 1), (FL.HOST, 1, 2), (FL.HOST, 2, 1), (FL.HOST, 2, 2), (FL.HOST, 3, 1)} <= cells
    # each cap's two sides are cases of their own
    by_name = {}
    for name, g, cases in FL.hand_groups():
        if name == "own":
            for c in cases:
                by_name.setdefault(c["name"], []).append(c)
    for ok, refused, cell in (("kband_1033", "kband_1034", (FL.HOST, 5, 1)), ("window_256", "window_257", (FL.HOST, 5, 1))):
        assert all(c["answer"]["outcome"] == FL.DONE for c in by_name[ok] if c["tags"] & {"small_kband_31", "small_window_256"})
        hit = [c for c in by_name[refused] if c["tags"] & {"small_kband_32", "small_window_257"}]
        assert len(hit) >= FL.MIN_PER_TAG and all((c["answer"]["outcome"], c["answer"]["stage"], c["answer"]["detail"]) == cell for c in hit)
        assert {c["answer"]["refused"] for c in hit} == ({4} if ok == "kband_1033" else {2})
    grown = [c for c in by_name["grow_64"] if "grow_past_64" in c["tags"]]
    assert len(grown) >= FL.MIN_PER_TAG and all(len(c["exons"]) == 64 and len(c["answer"]["exons"]) == 65 for c in grown)


def test_the_cases_notice_three_wrong_ways_to_glue_the_stages():
    differ = {"tail_on_working": 0, "clean_on_working": 0, "keep_removed": 0}
    for name, g, cases in FL.hand_groups():
        ops = SL.OracleOps(g)
        for c in cases:
            for how in differ:
                if how != "keep_removed" and c["orig"] == c["est"]:
                    continue
                if how == "keep_removed" and not c["answer"]["n_removed"]:
                    continue
                differ[how] += FL._answer(c, g, ops, **{how: True})[0] != c["answer"]
    assert min(differ.values()) >= FL.MIN_PER_TAG, differ


def test_the_trivial_queries_ask_nothing():
    for name, g, cases in FL.hand_groups()[:2]:
        ops = SL.OracleOps(g)
        for c in cases[:20]:
            for seq in (c["est"], c["est"][:1]):
                info = {}
                t = TL.tail(c["orig"][:len(seq)], seq, g, [(0, len(seq) - 1, 0, 0)], info=info)
                assert t == (TL.OK, 0, 0, 0, 0, 1, 0, [(0, len(seq) - 1, 0, 0)], [0]), (c["name"], t)
                assert "refused" not in info and not any(k.startswith("dp_") for k in info), info
                info = {}
                s = SL.small(c["orig"][:len(seq)], seq, g, [(0, 0, 0, 0)], 40, ops=ops, info=info)
                assert s[0] == SL.OK and s[1] == 0 and s[3:6] == (0, 0, 1) and s[8] == [(0, 0, 0, 0)], (c["name"], s)
                asked = {k: v for k, v in info.items() if k.startswith("dp_")}
                assert "refused" not in info and asked == {"dp_kband": 1}, info      # the cleaning of one cell, verdict ignored


def test_binding_matches_the_header():
    from pintron_amd import capi
    import binding_lib as B
    names = ["pgpu_pairing_plan_create_with_originals", "pgpu_pairing_plan_run_final_factorizations", "pgpu_pairing_plan_final_exons",
             "pgpu_pairing_plan_fetch_final_factorizations", "pgpu_pairing_plan_final_ms", "pgpu_index_final_factorizations",
             "pgpu_index_final_factorizations_kernel_ms"]
    assert all(n in capi.EXPORTS for n in names)
    L = capi.lib()
    assert all(hasattr(L, n) for n in names) and L.pgpu_abi_version() == 1
    text = open(B.HEADER).read()
    size_of = dict(B.SIZE_OF, uint16_t=2, uint8_t=1)
    fields, size = B.header_struct("pgpu_final_result")
    dt = np.dtype(capi.FINAL_RESULT_DTYPE)
    assert [f for f, _ in fields] == [f for f, _ in capi.FinalResult._fields_] == [f for f, _ in capi.FINAL_RESULT_DTYPE]
    off, offsets = 0, []
    for f, ctype in fields:
        assert getattr(capi.FinalResult, f).offset == off == dt.fields[f][1], f
        assert getattr(capi.FinalResult, f).size == size_of[ctype] == dt.fields[f][0].itemsize, f
        offsets.append(off)
        off += size_of[ctype]
    assert off == size == 32 == C.sizeof(capi.FinalResult) == dt.itemsize
    assert offsets == [0, 1, 2, 4, 8, 10, 12, 16, 20, 21, 22, 23, 24, 26, 28, 30, 31]
    assert re.search(r"typedef pgpu_tail_query pgpu_final_query;", text) and capi.FinalQuery is capi.TailQuery
    assert capi.FINAL_QUERY_DTYPE == capi.TAIL_QUERY_DTYPE
    assert tuple(f for f in FL.FIELDS) == tuple(f for f, _ in capi.FINAL_RESULT_DTYPE if f not in ("first_exon", "n_exons", "reserved"))


def test_host_side_of_the_entries_under_sanitizers(tmp_path):
    exe = str(tmp_path / "final_call_check")                     # pgpu_final.h needs the C-ABI's header alone: no ROCm header
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(HERE, "hostcheck", "final_call_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == "ok\n", (r.stdout, r.stderr[-2000:])
