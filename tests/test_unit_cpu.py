"""CPU: the unit stage's restatement (tests/unit_lib.py) against the records the host program itself writes
(tests/hostcheck/estfact_sched_check under PINTRON_RECORDS_FILE) on the three real inputs, with retain_externals on and off;
ESTs whose graph is empty; the cover of the hand-made cases the GPU tests use and that they notice six wrong rules; the binding
against the header, the records' own reader over a restated blob, and the host side of the entries that makes no HIP call in a
stand-alone program under AddressSanitizer and UBSan."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import cand_lib as KL
import final_lib as FL
import unit_lib as UL

HERE = os.path.dirname(os.path.abspath(__file__))
# ALIGNED units that must be compared per input (the counts measured with the real originals: 151, 10 and 796; the margin is
# for outcomes that move to a cap of an earlier stage), and UNALIGNED ones
FLOORS = dict(c2=(140, 1), ambn=(8, 0), issue13=(750, 1))


@pytest.fixture(scope="module")
def program():
    subprocess.run(["make", "-s", "-C", os.path.join(HERE, "hostcheck"), "estfact_sched_check"], check=True)
    return os.path.join(HERE, "hostcheck", "estfact_sched_check")


@pytest.mark.parametrize("source", ["c2", "ambn", "issue13"])
def test_the_program_cpu(program, tmp_path, source):
    """final_lib.final per prepared sequence with the real originals, the restatement over them, and the groups the program
    wrote: every ALIGNED unit's group byte for byte, no group for an UNALIGNED unit, nothing but HOST units left out"""
    U = UL.real_units(source)
    gfa, efa = KL.real_inputs()[source]
    answers, empty = UL.real_finals(source)
    res, exons, _ = FL.expect_arrays(answers)
    q = UL.unit_queries(U)
    assert len(q) == len(U["fixed"]) and all((int(r) == UL.NO_SIBLING) == f for r, f in zip(q["rev"], U["fixed"]))
    theirs = {}
    for retain in (1, 0):
        theirs[retain] = UL.program_records(program, gfa, efa, retain, str(tmp_path / ("retain%d" % retain)), {"PINTRON_THREADS": "4"})
        out, blob = UL.units(res, exons, empty, q, U["pref_N"], retain)
        n_aligned, n_unaligned, wrong = UL.against_the_program(out, blob, q, theirs[retain])
        print("%s retain_externals %d: ALIGNED %d (fwd %d, rev %d), UNALIGNED %d, HOST %d, groups of the program %d, disagreements %d"
              % (source, retain, n_aligned, int(((out["verdict"] == 2) & (out["strand"] == 0)).sum()),
                 int(((out["verdict"] == 2) & (out["strand"] == 1)).sum()), n_unaligned, int((out["verdict"] == 0).sum()),
                 len(UL.read_blob(theirs[retain])), len(wrong)))
        assert not wrong, [(i, U["units"][i]) for i in wrong[:10]]
        assert n_aligned >= FLOORS[source][0] and n_unaligned >= FLOORS[source][1]
        # a call whose units are all settled is the program's blob for those ESTs
        settled = np.nonzero(out["verdict"] != UL.U_HOST)[0]
        mine = UL.units(res, exons, empty, q[settled], U["pref_N"], retain)[1]
        groups = UL.groups_by_index(theirs[retain])
        assert mine == b"".join(groups[int(q["est_index"][i])] for i in settled if out["verdict"][i] == UL.U_ALIGNED)
    assert theirs[0] != theirs[1]
    # the comparison notices the working sequence put in place of the originals
    if source != "ambn":
        a2, _ = UL.finals(gfa, efa, U, use_originals=False, base=answers)
        r2, e2, _ = FL.expect_arrays(a2)
        out, blob = UL.units(r2, e2, empty, q, U["pref_N"], 1)
        moved = UL.against_the_program(out, blob, q, theirs[1])[2]
        print("%s: the working sequence for the original moves %d units" % (source, len(moved)))
        assert len(moved) >= 1
    # the floors refuse a restatement without the empty-graph rule, and one without the sibling rule (c2 aligns on the
    # forward strand throughout: its two UNALIGNED units are what the empty-graph rule settles)
    def misses(n_aligned, n_unaligned, _):
        return n_aligned < FLOORS[source][0] or n_unaligned < FLOORS[source][1]
    out, blob = UL.units(res, exons, None, q, U["pref_N"], 1)
    assert misses(*UL.against_the_program(out, blob, q, theirs[1]))
    alone = q.copy()
    alone["rev"] = UL.NO_SIBLING
    out, blob = UL.units(res, exons, empty, alone, U["pref_N"], 1)
    assert source == "c2" or misses(*UL.against_the_program(out, blob, alone, theirs[1]))


def _no_common_15mer(rng, genomic, n):
    """a seeded sequence of n bases that shares no 15-mer with the genomic sequence on either strand"""
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    mers = {genomic[k:k + 15] for k in range(len(genomic) - 14)}
    while True:
        s = bytes(rng.choice(b"ACGT") for _ in range(n))
        rc = s.translate(comp)[::-1]
        if not any(x[k:k + 15] in mers for x in (s, rc) for k in range(n - 14)):
            return s


def test_the_empty_graph(program, tmp_path):
    """ESTs that share no 15-mer with the genomic sequence on either strand, one of them on a fixed strand, among real ones:
    the program writes no group for them, and the restatement says UNALIGNED by an empty graph"""
    gfa, efa = KL.real_inputs()["ambn"]
    blocks = [b for b in efa.split(">") if b]
    genomic = UL.real_units("ambn")["genomic"]
    rng = random.Random(411)
    made = [(">/gb=ZZ%06d /gi=%d /ug=Hs.0 /len=%d\n" % (k, k, n), _no_common_15mer(rng, genomic.upper(), n)) for k, n in enumerate((120, 300, 451))]
    made.append((">/gb=NM_999999 /gi=9 /ug=Hs.0 /len=260\n", _no_common_15mer(rng, genomic.upper(), 260)))     # a RefSeq: fixed strand
    # six real ESTs beside them, in input order: four the restatement settles and two it leaves to the host
    full, full_empty = UL.real_finals("ambn")
    fres, fex, _ = FL.expect_arrays(full)
    verdicts = UL.units(fres, fex, full_empty, UL.unit_queries(UL.real_units("ambn")))[0]["verdict"]
    keep = sorted(list(np.nonzero(verdicts == UL.U_ALIGNED)[0][:4]) + list(np.nonzero(verdicts == UL.U_HOST)[0][:2]))
    assert len(keep) == 6 and len(blocks) == len(verdicts)
    texts = [">" + blocks[i] for i in keep]
    where = {}
    for k, (head, seq) in enumerate(made):
        where[2 * k + 1] = head                          # between the real ones
        texts.insert(2 * k + 1, head + seq.decode() + "\n")
    efa2 = "".join(texts)
    U = UL.prepared(gfa, efa2)
    assert len(U["units"]) == 10 and sum(U["fixed"]) >= 1 and U["fixed"][7]
    answers, empty = UL.finals(gfa, efa2, U)
    res, exons, _ = FL.expect_arrays(answers)
    q = UL.unit_queries(U)
    out, blob = UL.units(res, exons, empty, q, U["pref_N"], 1)
    theirs = UL.program_records(program, gfa, efa2, 1, str(tmp_path / "run"), {"PINTRON_THREADS": "2"})
    n_aligned, n_unaligned, wrong = UL.against_the_program(out, blob, q, theirs)
    assert not wrong and n_aligned == 4 and n_unaligned == 4
    groups = UL.groups_by_index(theirs)
    for i in where:
        assert i not in groups
        assert (int(out["verdict"][i]), int(out["reason"][i])) == (UL.U_UNALIGNED, 2), (i, out[i])
        assert int(out["strand"][i]) == (0 if U["fixed"][i] else 1)
        for p in (int(q["fwd"][i]), int(q["rev"][i])):
            if p != UL.NO_SIBLING:
                assert empty[p] and (answers[p]["outcome"], answers[p]["stage"], answers[p]["detail"]) == (FL.HOST, 0, KL.NOT_PATH)


def test_the_cover_of_the_hand_made_cases():
    cases = UL.hand_cases()
    assert 100 <= len(cases) <= 400
    seen = set()
    for pref_N, retain in UL.SETTINGS:
        for c in cases:
            seen |= UL.tags_of(c, pref_N, retain)
    assert seen >= set(UL.TAGS), sorted(set(UL.TAGS) - seen)
    # units in another order than their patterns, and their exons in a third
    res, exons, empty, q = UL.batch(cases)
    out, blob = UL.units(res, exons, empty, q)
    decided = out["pattern"][out["verdict"] == UL.U_ALIGNED]
    assert np.any(np.diff(decided.astype(np.int64)) < 0) and np.any(q["rev"][q["rev"] != UL.NO_SIBLING] < q["fwd"][q["rev"] != UL.NO_SIBLING])
    assert {int(v) for v in out["verdict"]} == {0, 1, 2} and {int(v) for v in out["reason"]} == {0, 1, 2}
    assert {int(v) for v in out["strand"]} == {0, 1} and {int(v) for v in out["n_factorizations"]} == {0, 1}
    assert all(int(a) % 4 == 0 and int(n) % 4 == 0 for a, n in zip(out["first_byte"], out["n_bytes"]))
    walked = UL.read_blob(blob)
    assert [w[2] for w in walked] == [int(q["est_index"][i]) for i in range(len(q)) if out["verdict"][i] == UL.U_ALIGNED]
    assert max(len(f[2]) for w in walked for f in w[3]) == UL.MAX_EXONS


def test_the_cases_notice_wrong_rules():
    res, exons, empty, q = UL.batch(UL.hand_cases())
    differ = dict.fromkeys(UL.WRONG, 0)
    for pref_N, retain in UL.SETTINGS:
        out, blob = UL.units(res, exons, empty, q, pref_N, retain)
        for how in UL.WRONG:
            o2, b2 = UL.units(res, exons, empty, q, pref_N, retain, wrong=how)
            differ[how] += b2 != blob
    assert min(differ.values()) >= 1, differ


def test_binding_matches_the_header():
    from pintron_amd import capi
    import binding_lib as B
    names = ["pgpu_unit_records", "pgpu_unit_records_kernel_ms", "pgpu_pairing_plan_run_units", "pgpu_pairing_plan_unit_bytes",
             "pgpu_pairing_plan_fetch_units", "pgpu_pairing_plan_units_ms"]
    assert all(n in capi.EXPORTS for n in names)
    L = capi.lib()
    assert all(hasattr(L, n) for n in names) and L.pgpu_abi_version() == 1
    size_of = dict(B.SIZE_OF, uint8_t=1)
    for cname, struct, dtype, offsets in (("pgpu_unit_query", capi.UnitQuery, capi.UNIT_QUERY_DTYPE, [0, 4, 8, 12]),
                                          ("pgpu_unit_result", capi.UnitResult, capi.UNIT_RESULT_DTYPE, [0, 1, 2, 3, 4, 8, 16, 20])):
        fields, size = B.header_struct(cname)
        dt = np.dtype(dtype)
        assert [f for f, _ in fields] == [f for f, _ in struct._fields_] == [f for f, _ in dtype]
        off, seen = 0, []
        for f, ctype in fields:
            assert getattr(struct, f).offset == off == dt.fields[f][1], (cname, f)
            assert getattr(struct, f).size == size_of[ctype] == dt.fields[f][0].itemsize, (cname, f)
            seen.append(off)
            off += size_of[ctype]
        assert off == size == C.sizeof(struct) == dt.itemsize and seen == offsets
    fields, size = B.header_struct("pgpu_unit_params")
    assert fields == [("pref_N_length", "int32_t"), ("retain_externals", "uint8_t"), ("reserved[3]", "uint8_t")] and size == 8
    assert [f for f, _ in capi.UnitParams._fields_] == ["pref_N_length", "retain_externals", "reserved"]
    assert (capi.UnitParams.pref_N_length.offset, capi.UnitParams.retain_externals.offset, capi.UnitParams.reserved.offset,
            capi.UnitParams.reserved.size, C.sizeof(capi.UnitParams)) == (0, 4, 5, 3, 8)
    text = open(B.HEADER).read()
    for name, value in (("PGPU_UNIT_NO_SIBLING", "0xffffffffu"), ("PGPU_UNIT_FWD_SUFF_POLYA", "1u"), ("PGPU_UNIT_REV_SUFF_POLYA", "2u"),
                        ("PGPU_UNIT_HOST", "0u"), ("PGPU_UNIT_UNALIGNED", "1u"), ("PGPU_UNIT_ALIGNED", "2u")):
        assert "#define %s %s" % (name, value) in " ".join(text.split()), name
    assert (capi.UNIT_NO_SIBLING, capi.UNIT_FWD_SUFF_POLYA, capi.UNIT_REV_SUFF_POLYA) == (UL.NO_SIBLING, UL.FWD_SUFF, UL.REV_SUFF)
    assert (capi.UNIT_HOST, capi.UNIT_UNALIGNED, capi.UNIT_ALIGNED) == (UL.U_HOST, UL.U_UNALIGNED, UL.U_ALIGNED)


@pytest.fixture(scope="module")
def call_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("unit") / "unit_call_check")     # pgpu_unit.h needs the C-ABI's header alone: no ROCm header
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(HERE, "hostcheck", "unit_call_check.cpp")], check=True)
    return exe


def test_host_side_of_the_entries_under_sanitizers(call_check):
    r = subprocess.run([call_check], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == "ok\n", (r.stdout, r.stderr[-2000:])


def test_the_records_reader_walks_a_restated_blob(call_check, tmp_path):
    """include/pintron_records.h over the blob of the hand-made cases, under every setting: the same numbers to the end"""
    res, exons, empty, q = UL.batch(UL.hand_cases())
    for k, (pref_N, retain) in enumerate(UL.SETTINGS):
        out, blob = UL.units(res, exons, empty, q, pref_N, retain)
        path = tmp_path / ("blob%d.bin" % k)
        path.write_bytes(blob)
        r = subprocess.run([call_check, str(path)], capture_output=True, text=True)
        assert r.returncode == 0, (r.stdout[-500:], r.stderr[-2000:])
        want = []
        for _, _, est_index, facts in UL.read_blob(blob):
            nums = [est_index, len(facts)]
            for polya, polyad, ex in facts:
                nums += [polya, polyad, len(ex)] + [v for e in ex for v in e]
            want.append(" ".join(str(v) for v in nums))
        assert r.stdout.splitlines() == want
    cut = tmp_path / "cut.bin"
    cut.write_bytes(blob[:-4])
    r = subprocess.run([call_check, str(cut)], capture_output=True, text=True)
    assert r.returncode == 1 and r.stdout.splitlines()[-1] == "-1"
