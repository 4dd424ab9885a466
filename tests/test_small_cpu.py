"""CPU: the restatement of pgpu_index_small_chains (tests/small_lib.py) against the fixture that the reference's
refine_EST_factorizations, the restatement and the host's ef_chain_small agreed on (tests/golden/small_chains.json.gz), the
cover of that fixture, that the fixture notices the three wrong builds, the restatement against ef_chain_small on every
factorization of the three real inputs, the generator's yields, the cap rules of the restatement at their edges, the
binding's layout against the header, and the host side of the entry that makes no HIP call (the shared validator with the
entry's own rules, the parameters, the device layout with two output slots per exon) in a stand-alone program under
AddressSanitizer and UBSan."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import binding_lib as BL
import resource_lib
import small_lib as SL
import tail_lib as TL

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCES = ("c2", "ambn", "issue13")


def worlds_with_real():
    worlds, real = SL.load_fixture()
    return list(worlds) + [(TL.real_done(src)[0], real[src]) for src in SOURCES]


def test_restatement_equals_the_fixture_on_every_case():
    n = 0
    for g, cases in worlds_with_real():
        ops = SL.OracleOps(g)
        for c in cases:
            info = {"tagged": True}
            got = SL.small(c["orig"], c["est"], g, c["exons"], c["mil"], ops=ops, info=info)
            assert got == c["answer"], (c["name"], got, c["answer"])
            assert set(SL.tags_of(info)) == c["tags"] - {"outside"}, (c["name"], SL.tags_of(info), c["tags"])
            status, refused, verdict, prefix_added, n_added, n_list, first, kept, lst, steps = got
            if status == SL.ERANGE:
                assert refused in (1, 2, 3, 4, 5) and got[2:8] == (0,) * 6 and lst == c["exons"] and not any(steps)
            else:
                assert refused == 0 and len(lst) == len(steps) == n_list == len(c["exons"]) + n_added <= 2 * len(c["exons"])
                assert prefix_added == (steps[0] & SL.STEP_PREFIX) and n_added == sum(1 for s in steps if s & 3)
                assert (verdict == 0) == (kept > 0) and first + kept <= n_list
                assert all(bool(s & SL.STEP_EXTERNAL) <= (not first <= i < first + kept) for i, s in enumerate(steps))
            q = [dict(est_off=0, est_len=len(c["est"]), first_exon=0, n_exons=len(c["exons"]), reserved=0, orig_off=0)]
            assert not SL.einval(len(c["est"]), len(g), c["exons"], q), c["name"]
            n += 1
    assert n > 1200


def test_the_fixture_covers_what_it_must():
    worlds, real = SL.load_fixture()
    hand = [c for _, cases in worlds for c in cases]
    assert len(hand) >= 300 and all(1000 < len(g) < 1_000_000 for g, _ in worlds)
    tail_real = TL.load_fixture()[2]
    for src in SOURCES:                                       # the factorizations the tail fixture keeps, every one of them
        assert len(real[src]) == sum(1 for c in tail_real[src] if c["answer"][:2] == (TL.OK, 0))
    tags = {t: 0 for t in SL.TAGS}
    for c in hand + [c for v in real.values() for c in v]:
        assert c["tags"] <= set(SL.TAGS) | {"outside"}
        for t in c["tags"] & set(SL.TAGS):
            tags[t] += 1
    assert min(tags.values()) >= SL.MIN_PER_TAG, tags
    # every tag of a refusal is a refused case, and a case that carries no witness of the reference says why
    for c in hand:
        if c["tags"] & set(SL.REFUSED_TAGS):
            assert c["answer"][0] == SL.ERANGE, c["name"]
        assert 2 in c["witnesses"]
        if 1 not in c["witnesses"]:
            assert c["tags"] & {"outside", "disordered"}, c["name"]
    assert sum(1 in c["witnesses"] for c in hand) >= len(hand) - 20
    assert all(c["witnesses"] == [1, 2, 3] for v in real.values() for c in v)
    assert os.path.getsize(SL.FIXTURE) <= 1 << 20
    md = open(SL.FIXTURE[:-len(".json.gz")] + ".md").read()
    for t, n in tags.items():
        assert "`%s`: %d" % (t, n) in md, t


def test_the_fixture_notices_the_three_wrong_builds():
    worlds, _ = SL.load_fixture()
    for how in ("again", "clean_on_working", "external_first"):
        differ = 0
        for g, cases in worlds:
            ops = SL.OracleOps(g)
            differ += sum(SL.small(c["orig"], c["est"], g, c["exons"], c["mil"], ops=ops, **{how: True}) != c["answer"] for c in cases)
        assert differ >= SL.MIN_PER_TAG, (how, differ)


@pytest.mark.parametrize("source", SOURCES)
def test_restatement_equals_the_host_code_on_real_inputs(source):
    genomic = TL.real_done(source)[0]
    cases = SL.load_fixture()[1][source]
    assert len(cases) >= (100 if source != "ambn" else 5)
    host, ops = SL.Host(genomic), SL.OracleOps(genomic)
    try:
        for c in cases:                                       # the host has no caps
            for mil in (c["mil"], 4, 100):
                info = {"no_caps": True}
                mine = SL.small(c["orig"], c["est"], genomic, c["exons"], mil, ops=ops, info=info)
                if not info.get("outside"):
                    assert SL.agrees_with_host(mine, host.small(c["orig"], c["est"], c["exons"], mil)), (source, c["name"], mil, mine)
    finally:
        host.close()


def test_the_generator_yields_what_the_gpu_test_needs():
    g, batch = SL.generated(2026, 2000)
    ops = SL.OracleOps(g)
    want = [SL.small(o, e, g, ex, mil, ops=ops) for _, o, e, ex, mil in batch]
    assert all(w[0] == SL.OK for w in want)
    assert sum(w[3] for w in want) >= 200                     # prefix insertions
    assert sum(w[4] - w[3] > 0 for w in want) >= 200          # insertions between two exons
    assert sum(w[7] < w[5] for w in want) >= 200              # step 3 drops something


def _first(hand, tag):
    return next(c for c in hand if tag in c["tags"])


def test_caps_of_the_restatement_at_their_edges():
    worlds, _ = SL.load_fixture()
    where = {id(c): g for g, cases in worlds for c in cases}
    hand = [c for _, cases in worlds for c in cases]

    def free(c):
        return SL.small(c["orig"], c["est"], where[id(c)], c["exons"], c["mil"], info={"no_caps": True})
    # each cap: the last accepted and the first refused value, and a refusal leaves the exons as they came
    for ok_tag, refused_tag, code in (("grow_past_64", "exons_65", 1), ("window_256", "window_257", 2), ("piece_one_n", "piece_two_n", 3),
                                      ("at_first_bad", "past_first_bad", 3), ("kband_31", "kband_32", 4)):
        a, b = _first(hand, ok_tag), _first(hand, refused_tag)
        assert a["answer"][0] == SL.OK and b["answer"][:2] == (SL.ERANGE, code)
        assert b["answer"] == (SL.ERANGE, code, 0, 0, 0, 0, 0, 0, b["exons"], [0] * len(b["exons"]))
        assert free(b)[0] == SL.OK
    assert len(_first(hand, "grow_past_64")["exons"]) == 64 and _first(hand, "grow_past_64")["answer"][5] > 64
    assert len(_first(hand, "exons_65")["exons"]) == 65
    # order is a refusal with or without the caps (the reference asserts it)
    d = _first(hand, "disordered")
    assert d["answer"][:2] == (SL.ERANGE, 5) and free(d)[:2] == (SL.ERANGE, 5)
    # a cap refuses only when the computation it bounds would run: EST_start 6 asks nothing of the prefix, whatever lies there
    c = _first(hand, "est_start_6")
    assert c["answer"][0] == SL.OK and c["answer"][3] == 0
    # splice sites that are no upper-case GT .. AG.  IN FRONT of the first exon they put that exon behind the first byte that
    # is no upper-case ACGT: refused = 3 (with the caps lifted the lower-case pair is canonical, the mixed-case one is not).
    # AT the exon's start -- the exon laid over a short intron -- GEN_start is that first byte and the query is answered:
    # the lower-case pair gives the insertion, the mixed-case one none
    low, mixed = (next(c for c in hand if c["name"] == n) for n in ("site_lower", "site_mixed"))
    assert low["answer"][:2] == mixed["answer"][:2] == (SL.ERANGE, 3)
    info = {"no_caps": True}
    a = SL.small(low["orig"], low["est"], where[id(low)], low["exons"], low["mil"], info=info)
    assert info.get("lower_gtag") and a[3] == 1
    info = {"no_caps": True}
    a = SL.small(mixed["orig"], mixed["est"], where[id(mixed)], mixed["exons"], mixed["mil"], info=info)
    assert info.get("not_canonical") and a[3] == 0
    lows, mixeds = ([c for c in hand if c["name"] == n] for n in ("gtag_lower", "gtag_mixed"))
    assert len(lows) >= SL.MIN_PER_TAG and len(mixeds) >= SL.MIN_PER_TAG
    for c in lows:
        assert c["answer"][0] == SL.OK and c["answer"][3] == 1 and {"lower_gtag", "at_first_bad"} <= c["tags"] and 1 in c["witnesses"]
        new, moved = c["answer"][8][:2]
        assert where[id(c)][new[3] + 1:new[3] + 3] == b"gt" and where[id(c)][moved[2] - 2:moved[2]] == b"ag"
        assert {c["mil"] for c in lows} == {0, 4}
    for c in mixeds:
        assert c["answer"][0] == SL.OK and c["answer"][3] == 0 and {"mixed_gtag", "not_canonical"} <= c["tags"] and 1 in c["witnesses"]
    # the parameters
    c = hand[0]
    q = [dict(est_off=0, est_len=len(c["est"]), first_exon=0, n_exons=len(c["exons"]), reserved=0, orig_off=0)]
    assert SL.einval(len(c["est"]), len(where[id(c)]), c["exons"], q, params_reserved=1)


def test_binding_matches_the_header():
    from pintron_amd import capi
    assert "pgpu_index_small_chains" in capi.EXPORTS and "pgpu_index_small_chains_kernel_ms" in capi.EXPORTS
    L = capi.lib()
    assert hasattr(L, "pgpu_index_small_chains") and hasattr(L, "pgpu_index_small_chains_kernel_ms")
    assert L.pgpu_abi_version() == 1
    text = open(BL.HEADER).read()
    for name, mine, theirs in (("MAX_EXONS", capi.SMALL_MAX_EXONS, SL.MAX_EXONS),
                               ("MAX_PREFIX_WINDOW", capi.SMALL_MAX_PREFIX_WINDOW, SL.MAX_PREFIX_WINDOW),
                               ("MAX_KBAND", capi.SMALL_MAX_KBAND, SL.MAX_KBAND)):
        assert int(re.search(r"#define PGPU_SMALL_%s\s+(\d+)" % name, text).group(1)) == mine == theirs, name
    assert re.search(r"typedef pgpu_tail_query pgpu_small_query;", text) and capi.SmallQuery is capi.TailQuery
    assert capi.SMALL_QUERY_DTYPE == capi.TAIL_QUERY_DTYPE
    # the host code's constants are the same
    src = open(os.path.join(resource_lib.ROOT, "pintron_amd", "host", "ef_factref.c")).read()
    for name, mine in (("LB_SMALL_EXON", SL.LB), ("UB_SMALL_EXON", SL.UB), ("MIN_PERFECT_BORDER", SL.MPB)):
        assert int(re.search(r"#define %s (\d+)" % name, src).group(1)) == mine
    BL.assert_layout("pgpu_small_params", capi.SmallParams, capi.SMALL_PARAMS_DTYPE)
    # pgpu_small_result has 8-bit fields
    size_of = dict(BL.SIZE_OF, uint8_t=1)
    fields, size = BL.header_struct("pgpu_small_result")
    dt = np.dtype(capi.SMALL_RESULT_DTYPE)
    assert [f for f, _ in fields] == [f for f, _ in capi.SmallResult._fields_] == [f for f, _ in capi.SMALL_RESULT_DTYPE]
    off = 0
    for f, ctype in fields:
        assert getattr(capi.SmallResult, f).offset == off == dt.fields[f][1], f
        assert getattr(capi.SmallResult, f).size == size_of[ctype] == dt.fields[f][0].itemsize, f
        off += size_of[ctype]
    assert off == size == 24 == C.sizeof(capi.SmallResult) == dt.itemsize


def test_the_host_witness_is_built_into_the_check_library():
    import cand_lib as KL
    H = KL.host_lib()
    assert hasattr(H, "ef_chain_small") and hasattr(H, "ef_refine_last_steps")


def test_host_side_of_the_entry_under_sanitizers(tmp_path):
    hipcc = resource_lib.hipcc()
    if not hipcc:
        pytest.skip("no ROCm headers here")
    include = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "include")
    exe = str(tmp_path / "small_call_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", "-I" + include, "-o", exe,
                    os.path.join(HERE, "hostcheck", "small_call_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == "ok\n", (r.stdout, r.stderr[-2000:])
