"""CPU: the text stage's restatement (tests/text_lib.py) against the two files the host program itself writes
(tests/hostcheck/estfact_sched_check under PINTRON_RECORDS_FILE) on the three real inputs, with retain_externals on and off,
whole files; the same blobs through tests/hostcheck/records_to_text; that the comparison notices five wrong rules; the cover of
the hand-made cases the GPU tests use; the binding against the header; and the host side of the entries that makes no HIP
call in a stand-alone program under AddressSanitizer and UBSan."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cand_lib as KL
import text_lib as TL
import unit_lib as UL

HERE = os.path.dirname(os.path.abspath(__file__))
FLOORS = dict(c2=151, ambn=25, issue13=930)              # groups that must be compared per input


@pytest.fixture(scope="module")
def program():
    subprocess.run(["make", "-s", "-C", os.path.join(HERE, "hostcheck"), "estfact_sched_check", "records_to_text"], check=True)
    return os.path.join(HERE, "hostcheck", "estfact_sched_check")


def restated(rec, pests_file, genomic):
    """the restatement over a run's records, the sequences of its processed-ests.txt and the original genomic"""
    units, _ = TL.units_of_blob(rec)
    headers, seqs = TL.entries(pests_file)
    assert len(headers) == len(units)
    return TL.texts(units, rec, headers, seqs, genomic)


@pytest.mark.parametrize("source", ["c2", "ambn", "issue13"])
def test_the_program_cpu(program, tmp_path, source):
    gfa, efa = KL.real_inputs()[source]
    genomic = TL.original_genomic(gfa)
    ids = TL.est_headers(efa)
    seen = {}
    for retain in (1, 0):
        d = str(tmp_path / ("retain%d" % retain))
        rec, raw, pests = TL.program_texts(program, gfa, efa, retain, d, {"PINTRON_THREADS": "4"})
        out, my_raw, my_pests = restated(rec, pests, genomic)
        print("%s retain_externals %d: %d groups, raw %d bytes, processed-ests %d bytes" % (source, retain, len(out), len(raw), len(pests)))
        assert len(out) >= FLOORS[source] and (out["verdict"] == TL.DONE).all()
        assert my_raw == raw                                 # as a whole file
        assert my_pests == pests
        # the headers are those of ests.txt at the groups' est_index
        units, index = TL.units_of_blob(rec)
        assert TL.entries(pests)[0] == [ids[i] for i in index]
        # the same blobs through the host's own routine (ef_raw_text_from_records)
        r = subprocess.run([os.path.join(HERE, "hostcheck", "records_to_text"), "records.bin", "processed-ests.txt", "genomic.txt"],
                           cwd=d, capture_output=True)
        assert r.returncode == 0 and r.stdout == raw, r.stderr[-500:]
        # the files cut per group are the restated texts per unit
        cut = TL.per_est(rec, raw, pests)
        for i, idx in enumerate(index):
            a, n, b, m = (int(out[f][i]) for f in ("raw_first", "raw_bytes", "pests_first", "pests_bytes"))
            assert cut[idx] == (my_raw[a:a + n], my_pests[b:b + m]), idx
        seen[retain] = raw
    assert seen[0] != seen[1]


def test_the_comparison_notices_the_working_sequence(program, tmp_path):
    """a stretch taken from the working sequence: test-issue-13 has ESTs whose two sequences differ inside an exon"""
    gfa, efa = KL.real_inputs()["issue13"]
    U = UL.real_units("issue13")
    rec, raw, pests = TL.program_texts(program, gfa, efa, 1, str(tmp_path / "run"), {"PINTRON_THREADS": "4"})
    units, _ = TL.units_of_blob(rec)
    headers, seqs = TL.entries(pests)
    working = {o: w for w, o in zip(U["working"], U["original"])}
    assert all(s in working for s in seqs)
    swapped = [working[s] for s in seqs]
    assert swapped != seqs
    assert TL.texts(units, rec, headers, seqs, TL.original_genomic(gfa))[1] == raw
    assert TL.texts(units, rec, headers, swapped, TL.original_genomic(gfa))[1] != raw


def test_the_comparison_notices_a_missing_N_prefix(program, tmp_path):
    """genomic coordinates without the N prefix: test-AMBN behind 37 leading Ns"""
    gfa, efa = KL.real_inputs()["ambn"]
    head, _, body = gfa.partition("\n")
    gfa2 = head + "\n" + "N" * 37 + body
    rec, raw, pests = TL.program_texts(program, gfa2, efa, 1, str(tmp_path / "run"), {"PINTRON_THREADS": "4"})
    genomic = TL.original_genomic(gfa2)
    assert genomic.startswith(b"N" * 37) and genomic[37:38] != b"N"
    out, my_raw, my_pests = restated(rec, pests, genomic)
    assert len(out) >= FLOORS["ambn"] and my_raw == raw and my_pests == pests
    assert restated(rec, pests, genomic[37:])[1] != raw


@pytest.fixture(scope="module")
def hand():
    cases = TL.hand_cases()
    return cases, TL.batch(cases)


def test_the_cases_notice_clipping_left_out(hand):
    want = TL.texts(*hand[1], TL.genomic())
    assert TL.texts(*hand[1], TL.genomic(), wrong="no_clip")[1] != want[1]


def test_the_cases_notice_unsigned_numbers(hand):
    want = TL.texts(*hand[1], TL.genomic())
    assert TL.texts(*hand[1], TL.genomic(), wrong="unsigned")[1] != want[1]


def test_the_cases_notice_blobs_in_pattern_order(hand):
    want = TL.texts(*hand[1], TL.genomic())
    got = TL.texts(*hand[1], TL.genomic(), wrong="pattern_order")
    assert got[1] != want[1] and got[2] != want[2] and len(got[1]) == len(want[1])


def test_the_cover_of_the_hand_made_cases(hand):
    cases, (units, blob, headers, seqs) = hand
    assert 150 <= len(cases) <= 400
    seen = set()
    for c in cases:
        seen |= TL.tags_of(c)
    assert seen >= set(TL.TAGS), sorted(set(TL.TAGS) - seen)
    want = TL.texts(units, blob, headers, seqs, TL.genomic())
    assert {int(v) for v in want[0]["verdict"]} == {TL.NONE, TL.DONE}
    # every source offset, destination offset and length of a stretch
    moved = TL.stretches(units, blob, headers, seqs, want[0])
    missing = [(s, d, n) for n in TL.LENGTHS if n for s in range(4) for d in range(4) if (s, d, n) not in moved]
    assert not missing, missing[:20]
    assert {d for s, d, n in moved if n == 0} == {0, 1, 2, 3}
    # units, patterns and groups in three different orders
    aligned = units["verdict"] == UL.U_ALIGNED
    assert np.any(np.diff(units["pattern"].astype(np.int64)) < 0) and np.any(np.diff(units["first_byte"][aligned].astype(np.int64)) < 0)
    assert np.any(np.argsort(units["pattern"][aligned]) != np.argsort(units["first_byte"][aligned]))
    # header lengths 0-7, and a NONE unit between two DONE ones
    assert {len(h) for h in headers} >= set(range(8))
    v = [int(x) for x in want[0]["verdict"]]
    assert any(v[i - 1] == TL.DONE and v[i] == TL.NONE and v[i + 1] == TL.DONE for i in range(1, len(v) - 1))
    # the cap: exactly 2^24 bytes is DONE, a byte over is HOST, pests alone can pass it
    cap = TL.cap_cases()
    o, raw, pests = TL.texts(*TL.batch(cap), TL.genomic())
    by = {c["name"]: (int(o["verdict"][i]), int(o["raw_bytes"][i]), int(o["pests_bytes"][i])) for i, c in enumerate(cap)}
    assert by["cap_exact"][:2] == (TL.DONE, TL.MAX_UNIT_BYTES) and by["cap_one_over"] == (TL.HOST, 0, 0)
    assert by["cap_pests_alone"] == (TL.HOST, 0, 0) and by["cap_pests_exact"][0] == TL.DONE and by["cap_pests_exact"][2] == TL.MAX_UNIT_BYTES
    assert all(by["cap_neighbour_%d" % k][0] == TL.DONE for k in (1, 2, 3))
    assert len(TL.raw_of(cap[2]["header"], cap[2]["facts"], cap[2]["seq"], TL.genomic())) == TL.MAX_UNIT_BYTES + 1


def test_binding_matches_the_header():
    from pintron_amd import capi
    import binding_lib as B
    names = ["pgpu_text_source_create", "pgpu_text_source_destroy", "pgpu_unit_texts", "pgpu_unit_texts_kernel_ms",
             "pgpu_pairing_plan_run_texts", "pgpu_pairing_plan_text_bytes", "pgpu_pairing_plan_fetch_texts", "pgpu_pairing_plan_texts_ms",
             "pgpu_pairing_plan_texts_write_ms"]
    assert all(n in capi.EXPORTS for n in names)
    L = capi.lib()
    assert all(hasattr(L, n) for n in names) and L.pgpu_abi_version() == 1
    fields, size = B.header_struct("pgpu_text_result")
    assert fields == [("raw_first", "uint64_t"), ("pests_first", "uint64_t"), ("raw_bytes", "uint32_t"), ("pests_bytes", "uint32_t"),
                      ("verdict", "uint8_t"), ("reserved[7]", "uint8_t")] and size == 32
    dt = np.dtype(capi.TEXT_RESULT_DTYPE)
    names = ["raw_first", "pests_first", "raw_bytes", "pests_bytes", "verdict", "reserved"]
    assert [f for f, _ in capi.TextResult._fields_] == names == list(dt.names)
    for f, off, n in zip(names, (0, 8, 16, 20, 24, 25), (8, 8, 4, 4, 1, 7)):
        assert (getattr(capi.TextResult, f).offset, getattr(capi.TextResult, f).size) == (off, n) == (dt.fields[f][1], dt.fields[f][0].itemsize), f
    assert C.sizeof(capi.TextResult) == dt.itemsize == 32
    text = " ".join(open(B.HEADER).read().split())
    for name, value in (("PGPU_TEXT_NONE", "0u"), ("PGPU_TEXT_DONE", "1u"), ("PGPU_TEXT_HOST", "2u"), ("PGPU_TEXT_MAX_UNIT_BYTES", "(1u << 24)")):
        assert "#define %s %s" % (name, value) in text, name
    assert (capi.TEXT_NONE, capi.TEXT_DONE, capi.TEXT_HOST, capi.TEXT_MAX_UNIT_BYTES) == (TL.NONE, TL.DONE, TL.HOST, TL.MAX_UNIT_BYTES)


def test_host_side_of_the_entries_under_sanitizers(tmp_path):
    exe = str(tmp_path / "text_call_check")              # pgpu_text.h needs the C-ABI's header alone: no ROCm header
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(HERE, "hostcheck", "text_call_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == "ok\n", (r.stdout, r.stderr[-2000:])
