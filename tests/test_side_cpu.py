"""CPU: the side stage's restatement (tests/side_lib.py) against the three side files the host program itself writes
(tests/hostcheck/estfact_sched_check: megs.txt, processed-megs.txt, meg-edges.txt) on the three real inputs, EST by EST, for
every unit the restatement settles -- its inputs are the unit table of hostcheck/unit_prep_main, the verdicts of unit_lib
over final_lib.final and the first-attempt texts of hostcheck/meg_check, whose `@@complex 1` entries count as flagged; that
the comparison notices five wrong rules; the cover of the hand-made cases the GPU tests use; the binding against the header;
and the host side of the entry that makes no HIP call in a stand-alone program under AddressSanitizer and UBSan."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cand_lib as KL
import final_lib as FL
import meg_lib as M
import side_lib as SL
import text_lib as TL
import unit_lib as UL

HERE = os.path.dirname(os.path.abspath(__file__))
# units that must be compared per input: (ALIGNED, UNALIGNED) -- the floors tests/test_unit_cpu.py asserts for the same
# restated verdicts on these inputs
FLOORS = dict(c2=(140, 1), ambn=(8, 0), issue13=(750, 1))


@pytest.fixture(scope="module")
def program():
    subprocess.run(["make", "-s", "-C", os.path.join(HERE, "hostcheck"), "estfact_sched_check"], check=True)
    return os.path.join(HERE, "hostcheck", "estfact_sched_check")


_runs = {}


def real(source, program, tmp_path_factory):
    """(q, units, records, headers, originals, working, the program's files cut per EST) of a real input; once per process"""
    if source not in _runs:
        gfa, efa = KL.real_inputs()[source]
        U = UL.real_units(source)
        answers, empty = UL.real_finals(source)
        res, exons, _ = FL.expect_arrays(answers)
        q = UL.unit_queries(U)
        units, _ = UL.units(res, exons, empty, q, U["pref_N"], 1)
        exp, _ = M.first_attempt_megs(gfa, efa, M.DEFAULTS)
        assert [e["seq"] for e in exp] == U["working"]
        records = []
        for e in exp:
            verts, adj = KL.graph_of_meg_text(e["meg"])
            records.append(KL.bare(KL.UNAVAILABLE) if len(verts) > KL.MAX_VERTICES else
                           KL.record(verts, adj, KL.TOO_COMPLEX if e["complex"] else 0, e["meg"], e["edges"]))
        ids = TL.est_headers(efa)
        headers = [ids[int(i)] for i in q["est_index"]]
        d = str(tmp_path_factory.mktemp("side_" + source))
        UL.program_records(program, gfa, efa, 1, d, {"PINTRON_THREADS": "4"})
        files = SL.program_sides(d)
        _runs[source] = (q, units, records, headers, U["original"], U["working"], SL.per_est(ids, *files), files)
    return _runs[source]


def compared(q, units, got, theirs):
    """every DONE unit's three texts against the program's for that EST -> (ALIGNED compared, of them on the sibling,
    UNALIGNED compared, of them with a sibling, [units that disagree])"""
    out, blobs = got[0], got[1:]
    n = [0, 0, 0, 0]
    wrong = []
    for i in np.nonzero(out["verdict"] == SL.DONE)[0]:
        mine = tuple(blobs[k][int(out[f + "_first"][i]):int(out[f + "_first"][i]) + int(out[f + "_bytes"][i])]
                     for k, f in enumerate(("megs", "pmegs", "edges")))
        if theirs[int(q["est_index"][i])] != mine:
            wrong.append(int(i))
        aligned, strand = int(units["verdict"][i]) == UL.U_ALIGNED, int(units["strand"][i])
        n[0 if aligned else 2] += 1
        n[1 if aligned else 3] += strand
    return n[0], n[1], n[2], n[3], wrong


@pytest.mark.parametrize("source", ["c2", "ambn", "issue13"])
def test_the_program_cpu(program, tmp_path_factory, source):
    q, units, records, headers, originals, working, theirs, files = real(source, program, tmp_path_factory)
    got = SL.sides(q, units, records, headers, originals)
    n_al, n_al_rev, n_un, n_un_rev, wrong = compared(q, units, got, theirs)
    n_host = int((units["verdict"] == UL.U_HOST).sum())
    print("%s: ALIGNED %d (on the sibling %d), UNALIGNED %d (with a sibling %d), HOST %d, SIDE_HOST %d, disagreements %d; megs %d, pmegs %d, edges %d bytes"
          % (source, n_al, n_al_rev, n_un, n_un_rev, n_host, int((got[0]["verdict"] == SL.HOST).sum()), len(wrong), len(got[1]), len(got[2]), len(got[3])))
    assert not wrong, wrong[:10]
    assert n_al >= FLOORS[source][0] and n_un >= FLOORS[source][1]
    # every settled unit is DONE: no record a settled unit names is flagged, none is beyond the rule
    assert int((got[0]["verdict"] == SL.DONE).sum()) == len(units) - n_host and not (got[0]["verdict"] == SL.HOST).any()
    if source != "ambn":
        assert n_un_rev >= 1                             # UNALIGNED with a sibling: two entries of megs.txt
    if source == "issue13":
        assert n_al_rev >= 1                             # ALIGNED on the sibling (c2 and test-AMBN have none)
    # a call whose units are all settled is the program's files for those ESTs
    settled = np.nonzero(units["verdict"] != UL.U_HOST)[0]
    mine = SL.sides(q[settled], units[settled], records, [headers[i] for i in settled], originals)
    for k in range(3):
        assert mine[1 + k] == b"".join(theirs[int(q["est_index"][i])][k] for i in settled)
    if n_host == 0:
        assert mine[1:] == files


@pytest.fixture(scope="module")
def issue13(program, tmp_path_factory):
    return real("issue13", program, tmp_path_factory)


def test_the_comparison_notices_the_working_sequence(issue13):
    q, units, records, headers, originals, working, theirs, _ = issue13
    assert originals != working
    assert compared(q, units, SL.sides(q, units, records, headers, working), theirs)[4]


@pytest.mark.parametrize("wrong", SL.WRONG)
def test_the_comparison_notices_a_wrong_rule(issue13, wrong):
    """a sibling's entry left out of megs.txt when the forward strand fails; one added when the forward strand aligns; pmegs
    taken from the forward pattern on a strand-1 unit; blobs in pattern order"""
    q, units, records, headers, originals, working, theirs, _ = issue13
    if wrong == "pattern_order":                         # the patterns are in unit order in a prepared input: turn the units round
        q, units, headers = q[::-1].copy(), units[::-1].copy(), headers[::-1]
    good = SL.sides(q, units, records, headers, originals)
    assert not compared(q, units, good, theirs)[4]
    bad = SL.sides(q, units, records, headers, originals, wrong=wrong)
    if wrong == "pattern_order":
        # each unit's bytes are right and in the wrong place: the blobs as wholes differ, the offsets differ
        assert all(len(bad[k]) == len(good[k]) and bad[k] != good[k] for k in (1, 2, 3))
        assert (bad[0]["megs_first"] != good[0]["megs_first"]).any()
    else:
        assert compared(q, units, bad, theirs)[4]


@pytest.fixture(scope="module")
def hand():
    cases = SL.hand_cases()
    return cases, SL.batch(cases)


def test_the_cover_of_the_hand_made_cases(hand):
    cases, (q, units, records, headers, seqs) = hand
    assert 100 <= len(cases) <= 500, len(cases)
    seen = set()
    for c in cases:
        seen |= SL.tags_of(c)
    assert seen >= set(SL.TAGS), sorted(set(SL.TAGS) - seen)
    want = SL.sides(q, units, records, headers, seqs)
    assert {int(v) for v in want[0]["verdict"]} == {SL.NONE, SL.DONE, SL.HOST}
    # every source offset, destination offset and length of every kind of stretch, from the batch as it is laid out
    moved = SL.stretches(q, units, records, headers, seqs, want[0])
    missing = sorted(SL.needed_stretches() - moved)
    assert not missing, missing[:20]
    # units and patterns in different orders, records of different sizes at multiples of 4
    pats = units["pattern"].astype(np.int64)
    assert np.any(np.diff(pats) < 0) and np.any(np.diff(q["fwd"].astype(np.int64)) < 0)
    assert all(len(r) % 4 == 0 for r in records) and len({len(r) for r in records}) > 20
    # header lengths 0-7, and a NONE unit between two DONE ones
    assert {len(h) for h in headers} >= set(range(8))
    v = [int(x) for x in want[0]["verdict"]]
    assert any(v[i - 1] == SL.DONE and v[i] == SL.NONE and v[i + 1] == SL.DONE for i in range(1, len(v) - 1))
    # the four wrong rules are noticed on the cases too
    for wrong in SL.WRONG:
        bad = SL.sides(q, units, records, headers, seqs, wrong=wrong)
        assert any(bad[k] != want[k] for k in (1, 2, 3)), wrong
    # the cap: exactly 2^24 bytes is DONE, a byte over is HOST, pmegs past it is HOST
    cap = SL.cap_cases()
    o = SL.sides(*SL.batch(cap))[0]
    by = {c["name"]: (int(o["verdict"][i]), int(o["megs_bytes"][i]), int(o["pmegs_bytes"][i])) for i, c in enumerate(cap)}
    assert by["cap_exact"] == (SL.DONE, SL.MAX_UNIT_BYTES, 0) and by["cap_one_over"] == (SL.HOST, 0, 0)
    assert by["cap_pmegs_exact_megs_over"] == (SL.HOST, 0, 0) and by["cap_pmegs_alone"] == (SL.HOST, 0, 0)
    assert by["cap_megs_exact"] == (SL.DONE, SL.MAX_UNIT_BYTES, SL.MAX_UNIT_BYTES - 15)
    assert all(by["cap_neighbour_%d" % k][0] == SL.DONE for k in (1, 2, 3))
    c = cap[2]
    assert len(SL.unit_sides(c["verdict"], 1, 0, 1, c["header"], [c["f"]["rec"], c["r"]["rec"]], [c["f"]["seq"], c["r"]["seq"]])[0]) == SL.MAX_UNIT_BYTES + 1


def test_the_record_builder_prints_what_the_host_prints(program, tmp_path_factory):
    """meg_text and edges_text over the graph of every first-attempt text of c2 are those texts"""
    gfa, efa = KL.real_inputs()["c2"]
    exp, _ = M.first_attempt_megs(gfa, efa, M.DEFAULTS)
    n_edges = 0
    for e in exp:
        verts, adj = KL.graph_of_meg_text(e["meg"])
        assert SL.meg_text(verts, adj) == e["meg"] and SL.edges_text(verts, adj) == e["edges"]
        n_edges += e["edges"].count(b"\n")
    assert len(exp) >= 300 and n_edges >= 300


def test_binding_matches_the_header():
    from pintron_amd import capi
    import binding_lib as B
    names = ["pgpu_unit_sides", "pgpu_unit_sides_kernel_ms", "pgpu_pairing_plan_run_sides", "pgpu_pairing_plan_side_bytes",
             "pgpu_pairing_plan_fetch_sides", "pgpu_pairing_plan_sides_ms", "pgpu_pairing_plan_sides_write_ms"]
    assert all(n in capi.EXPORTS for n in names)
    L = capi.lib()
    assert all(hasattr(L, n) for n in names) and L.pgpu_abi_version() == 1
    fields, size = B.header_struct("pgpu_side_result")
    assert fields == [("megs_first", "uint64_t"), ("pmegs_first", "uint64_t"), ("edges_first", "uint64_t"), ("megs_bytes", "uint32_t"),
                      ("pmegs_bytes", "uint32_t"), ("edges_bytes", "uint32_t"), ("verdict", "uint8_t"), ("reserved[3]", "uint8_t")] and size == 40
    dt = np.dtype(capi.SIDE_RESULT_DTYPE)
    names = ["megs_first", "pmegs_first", "edges_first", "megs_bytes", "pmegs_bytes", "edges_bytes", "verdict", "reserved"]
    assert [f for f, _ in capi.SideResult._fields_] == names == list(dt.names)
    for f, off, n in zip(names, (0, 8, 16, 24, 28, 32, 36, 37), (8, 8, 8, 4, 4, 4, 1, 3)):
        assert (getattr(capi.SideResult, f).offset, getattr(capi.SideResult, f).size) == (off, n) == (dt.fields[f][1], dt.fields[f][0].itemsize), f
    assert C.sizeof(capi.SideResult) == dt.itemsize == 40
    text = " ".join(open(B.HEADER).read().split())
    for name, value in (("PGPU_SIDE_NONE", "0u"), ("PGPU_SIDE_DONE", "1u"), ("PGPU_SIDE_HOST", "2u"), ("PGPU_SIDE_MAX_UNIT_BYTES", "(1u << 24)")):
        assert "#define %s %s" % (name, value) in text, name
    assert (capi.SIDE_NONE, capi.SIDE_DONE, capi.SIDE_HOST, capi.SIDE_MAX_UNIT_BYTES) == (SL.NONE, SL.DONE, SL.HOST, SL.MAX_UNIT_BYTES)


def test_host_side_of_the_entries_under_sanitizers(tmp_path):
    exe = str(tmp_path / "side_call_check")              # pgpu_side.h needs the C-ABI's header alone: no ROCm header
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(HERE, "hostcheck", "side_call_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == "ok\n", (r.stdout, r.stderr[-2000:])
