"""CPU: the restatement of pgpu_index_tail_chains (tests/tail_lib.py) against the fixture that the reference's object code,
the restatement and the host's ef_chain_tail agreed on (tests/golden/tail_chains.json.gz), the cover of that fixture, the
restatement against ef_chain_tail on every DONE factorization of the three real inputs, the cap and PGPU_EINVAL rules of the
restatement at their edges, the binding's layout against the header, and the host side of the entry that makes no HIP call
(the shared validator with the entry's own rules, the device layout) in a stand-alone program under AddressSanitizer and
UBSan."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import binding_lib as BL
import resource_lib
import tail_lib as TL

HERE = os.path.dirname(os.path.abspath(__file__))


def real_genomic(source):
    return TL.real_done(source)[0]


def test_restatement_equals_the_fixture_on_every_case():
    gen, hand, real = TL.load_fixture()
    worlds = [(gen, hand)] + [(real_genomic(src), real[src]) for src in ("c2", "ambn", "issue13")]
    n = 0
    for g, cases in worlds:
        for c in cases:
            info = {"tagged": True}
            got = TL.tail(c["orig"], c["est"], g, c["exons"], info=info)
            assert got == c["answer"], (c["name"], got, c["answer"])
            assert set(TL.tags_of(info)) == c["tags"], (c["name"], TL.tags_of(info), c["tags"])
            status, verdict, polyA, polyadenil, recovered, kept, added, after, steps = got
            assert len(after) == len(steps) == len(c["exons"])
            if status == TL.ERANGE:
                assert got[1:7] == (0,) * 6 and after == c["exons"] and not any(steps)
            elif verdict:
                assert (recovered, kept) == (0, 0) and not any(steps) and after[:-1] == c["exons"][:-1]
            else:
                assert kept == sum(1 for s in steps if s & 3 != TL.REMOVED) >= 1
                assert bool(recovered & 1) == bool(steps[0] & TL.STEP_PREFIX) and bool(recovered & 2) == bool(steps[-1] & TL.STEP_SUFFIX)
                assert bool(added) == bool(steps[-1] & TL.STEP_TAIL)
            q = [dict(est_off=0, est_len=len(c["est"]), first_exon=0, n_exons=len(c["exons"]), reserved=0, orig_off=0)]
            assert not TL.einval(len(c["est"]), len(g), c["exons"], q), c["name"]
            n += 1
    assert n == len(hand) + sum(len(v) for v in real.values())


def test_the_fixture_covers_what_it_must():
    gen, hand, real = TL.load_fixture()
    assert len(gen) == TL.GEN_LEN and len(hand) >= 800
    assert {src: len(real[src]) for src in real} == {src: len(TL.real_done(src)[1]) for src in ("c2", "ambn", "issue13")}
    tags = {t: 0 for t in TL.TAGS}
    for c in hand + [c for v in real.values() for c in v]:
        assert c["tags"] <= set(TL.TAGS)
        for t in c["tags"]:
            tags[t] += 1
    assert min(tags.values()) >= TL.MIN_PER_TAG, tags
    # every tag of a refusal is a refused case, and every refused hand-made case has one
    for c in hand:
        assert (c["answer"][0] == TL.ERANGE) == bool(c["tags"] & set(TL.REFUSED_TAGS)), c["name"]
    assert os.path.getsize(TL.FIXTURE) <= 1 << 20
    md = open(TL.FIXTURE[:-len(".json.gz")] + ".md").read()
    for t, n in tags.items():
        assert "`%s`: %d" % (t, n) in md, t


def test_the_fixture_notices_a_walk_without_the_reanalysis_after_a_removal():
    gen, hand, _ = TL.load_fixture()
    differ = [c["name"] for c in hand if TL.tail(c["orig"], c["est"], gen, c["exons"], reanalyse=False) != c["answer"]]
    assert len(differ) >= TL.MIN_PER_TAG and differ.count("small_twice") >= TL.MIN_PER_TAG, differ


@pytest.mark.parametrize("source", ["c2", "ambn", "issue13"])
def test_restatement_equals_the_host_code_on_real_inputs(source):
    genomic, done = TL.real_done(source)
    assert len(done) >= (100 if source != "ambn" else 5)
    host = TL.Host(genomic)
    try:
        for k, (est, exons) in enumerate(done):                   # every DONE factorization: the host has no caps
            mine = TL.tail(est, est, genomic, exons, info={"no_caps": True})
            assert TL.agrees_with_host(mine, host.tail(est, est, exons)), (source, k, mine)
    finally:
        host.close()


def _query(est, ex, **kw):
    d = dict(est_off=0, est_len=len(est), first_exon=0, n_exons=len(ex), reserved=0, orig_off=0)
    d.update(kw)
    return d


def _first(hand, tag):
    return next(c for c in hand if tag in c["tags"])


def test_caps_and_einval_rules_of_the_restatement():
    gen, hand, _ = TL.load_fixture()
    glen = len(gen)
    # each cap: the last accepted and the first refused value, and a refusal leaves the exons as they came
    for ok_tag, refused_tag in (("exons_64", "exons_65"), ("affix_256", "affix_257"), ("window_128", "window_129"), ("gen_256", "gen_257")):
        a, b = _first(hand, ok_tag), _first(hand, refused_tag)
        assert a["answer"][0] == TL.OK and b["answer"][0] == TL.ERANGE
        assert b["answer"] == (TL.ERANGE, 0, 0, 0, 0, 0, 0, b["exons"], [0] * len(b["exons"]))
        assert TL.tail(b["orig"], b["est"], gen, b["exons"], info={"no_caps": True})[0] == TL.OK
    assert len(_first(hand, "exons_64")["exons"]) == 64 and len(_first(hand, "exons_65")["exons"]) == 65
    # a cap refuses only when its DP would run: 257 bytes in front of the exon whose first bytes are equal
    for side in ("pre", "suf"):
        c = next(c for c in hand if c["name"] == side + "_w257_skipped")
        assert c["answer"][0] == TL.OK and side + "_skipped" in c["tags"]
    # an exon of 101 EST bytes is not analysed, one of 100 is
    assert all(s & 3 == 0 for s in _first(hand, "exon_101")["answer"][8])
    assert _first(hand, "exon_100")["answer"][8][1] & 3 != 0
    # each bad query field
    c = next(c for c in hand if len(c["exons"]) >= 3 and c["answer"][:2] == (TL.OK, 0))
    est, ex = c["est"], c["exons"]
    assert not TL.einval(len(est), glen, ex, [_query(est, ex)])
    for bad in (_query(est, ex, n_exons=0), _query(est, ex, n_exons=len(ex) + 1), _query(est, ex, first_exon=1),
                _query(est, ex, first_exon=len(ex) + 1, n_exons=1), _query(est, ex, est_len=len(est) + 1), _query(est, ex, est_off=1),
                _query(est, ex, reserved=1), _query(est, ex, est_len=0), _query(est, ex, orig_off=1), _query(est, ex, orig_off=1 << 40)):
        assert TL.einval(len(est), glen, ex, [bad]), bad
    assert not TL.einval(2 * len(est), glen, ex, [_query(est, ex, orig_off=len(est))])           # the original behind the working one
    assert TL.einval(2 * len(est), glen, ex, [_query(est, ex, orig_off=len(est) + 1)])
    assert TL.einval(1 << 32, glen, ex, [_query(est, ex, est_len=1 << 31)])
    assert TL.einval(len(est), glen, ex, [_query(est, ex, n_exons=2), _query(est, ex, first_exon=1, n_exons=len(ex) - 1)])
    assert not TL.einval(len(est), glen, ex, [_query(est, ex, n_exons=2), _query(est, ex, first_exon=2, n_exons=len(ex) - 2)])
    # every coordinate a byte of its string: the last accepted and the first refused value
    for k, (low, high) in enumerate(((0, len(est) - 1), (0, len(est) - 1), (0, glen - 1), (0, glen - 1))):
        for v, bad in ((low, False), (high, False), (low - 1, True), (high + 1, True)):
            e2 = list(ex)
            e2[1] = tuple(v if i == k else x for i, x in enumerate(ex[1]))
            assert TL.einval(len(est), glen, e2, [_query(est, ex)]) == bad, (k, v)
    # order is no rule of the input: it is step 3's verdict
    for c in hand:
        if c["answer"][1] == 1:
            assert not TL.einval(len(c["est"]), glen, c["exons"], [_query(c["est"], c["exons"])])


def test_binding_matches_the_header():
    from pintron_amd import capi
    assert "pgpu_index_tail_chains" in capi.EXPORTS and "pgpu_index_tail_chains_kernel_ms" in capi.EXPORTS
    L = capi.lib()
    assert hasattr(L, "pgpu_index_tail_chains") and hasattr(L, "pgpu_index_tail_chains_kernel_ms")
    assert L.pgpu_abi_version() == 1
    text = open(BL.HEADER).read()
    for name, mine, theirs in (("MAX_EXONS", capi.TAIL_MAX_EXONS, TL.MAX_EXONS), ("MAX_AFFIX", capi.TAIL_MAX_AFFIX, TL.MAX_AFFIX),
                               ("MAX_SMALL_WINDOW", capi.TAIL_MAX_SMALL_WINDOW, TL.MAX_SMALL_WINDOW),
                               ("MAX_SMALL_GEN", capi.TAIL_MAX_SMALL_GEN, TL.MAX_SMALL_GEN),
                               ("UB_MED_EXON", capi.TAIL_UB_MED_EXON, TL.UB_MED_EXON),
                               ("AFFIXES_LENGTH", capi.TAIL_AFFIXES_LENGTH, TL.AFFIXES_LENGTH)):
        assert int(re.search(r"#define PGPU_TAIL_%s\s+(\d+)" % name, text).group(1)) == mine == theirs, name
    # the host code's constants are the same
    src = open(os.path.join(resource_lib.ROOT, "pintron_amd", "host", "ef_factref.c")).read()
    assert int(re.search(r"#define UB_MED_EXON (\d+)", src).group(1)) == TL.UB_MED_EXON
    assert int(re.search(r"#define AFFIXES_LENGTH (\d+)", src).group(1)) == TL.AFFIXES_LENGTH
    assert float(re.search(r"#define MAX_ERROR_RATE ([0-9.]+)", src).group(1)) == TL.MAX_ERROR_RATE
    BL.assert_layout("pgpu_tail_query", capi.TailQuery, capi.TAIL_QUERY_DTYPE)
    # pgpu_tail_result has 8-bit fields
    size_of = dict(BL.SIZE_OF, uint8_t=1)
    fields, size = BL.header_struct("pgpu_tail_result")
    dt = np.dtype(capi.TAIL_RESULT_DTYPE)
    assert [f for f, _ in fields] == [f for f, _ in capi.TailResult._fields_] == [f for f, _ in capi.TAIL_RESULT_DTYPE]
    off = 0
    for f, ctype in fields:
        assert getattr(capi.TailResult, f).offset == off == dt.fields[f][1], f
        assert getattr(capi.TailResult, f).size == size_of[ctype] == dt.fields[f][0].itemsize, f
        off += size_of[ctype]
    assert off == size == 16 == C.sizeof(capi.TailResult) == dt.itemsize
    assert np.dtype(capi.FACTOR_DTYPE).itemsize == C.sizeof(capi.Factor) == 16


def test_host_side_of_the_entry_under_sanitizers(tmp_path):
    hipcc = resource_lib.hipcc()
    if not hipcc:
        pytest.skip("no ROCm headers here")
    include = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "include")
    exe = str(tmp_path / "tail_call_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", "-I" + include, "-o", exe,
                    os.path.join(HERE, "hostcheck", "tail_call_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == "ok\n", (r.stdout, r.stderr[-2000:])
