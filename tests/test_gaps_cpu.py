"""CPU: the restatement of pgpu_index_gap_chains (tests/gaps_lib.py) against the fixture whose border refinements are the
reference's (tests/golden/gap_chains.json.gz), the cover of that fixture, the cap and PGPU_EINVAL rules of the restatement
at their edges, the binding's layout against the header, and the host side of the entry that makes no HIP call (the shared
validator with the entry's own rules, the device layout) in a stand-alone program under AddressSanitizer and UBSan."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import binding_lib as BL
import clean_lib as CL
import gaps_lib as GL
import resource_lib

HERE = os.path.dirname(os.path.abspath(__file__))


def test_restatement_equals_the_fixture_on_every_case():
    gen, cases = GL.load_fixture()
    for k, c in enumerate(cases):
        info = {}
        got = GL.gaps(c["est"], gen, c["exons"], info=info)
        assert got == (GL.OK, c["verdict"], c["total"], c["n_kept"], c["exons_after"], c["steps"]), (k, got, c)
        assert set(GL.tags_of(info)) == c["tags"], (k, info, c["tags"])
        assert (c["verdict"] == 1) == (c["total"] > GL.MAX_ERRORS) and (c["n_kept"] > 0) == (c["verdict"] == 0)
        assert c["n_kept"] == (len(c["exons"]) - sum(1 for s in c["steps"] if s & GL.MERGED) if c["verdict"] == 0 else 0)
        q = [dict(est_off=0, est_len=len(c["est"]), first_exon=0, n_exons=len(c["exons"]), reserved=0)]
        assert not GL.einval(len(c["est"]), len(gen), c["exons"], q), k


def test_the_fixture_covers_what_it_must():
    gen, cases = GL.load_fixture()
    assert len(gen) == GL.GEN_LEN and len(cases) >= 1000
    verdicts = [0, 0]
    tags = {t: 0 for t in ("merged", "merged_run", "short_window", "gap_equals_intron", "burset_tie", "total_20", "total_21",
                           "gap_64", "no_gap", "single_exon", "lower_or_N")}
    for c in cases:
        verdicts[c["verdict"]] += 1
        for t in tags:
            tags[t] += t in c["tags"]
        assert 1 <= len(c["exons"]) <= 6
    assert min(verdicts) >= 100, verdicts
    assert min(tags.values()) >= 25, tags
    assert os.path.getsize(GL.FIXTURE) <= os.path.getsize(CL.FIXTURE)
    md = open(GL.FIXTURE[:-len(".json.gz")] + ".md").read()
    for t, n in tags.items():
        assert "`%s`: %d" % (t, n) in md, t


def _query(est, ex, **kw):
    d = dict(est_off=0, est_len=len(est), first_exon=0, n_exons=len(ex), reserved=0)
    d.update(kw)
    return d


def test_caps_and_einval_rules_of_the_restatement():
    gen, cases = GL.load_fixture()
    glen = len(gen)
    refused = (GL.ERANGE, 0, 0, 0)
    # 64 / 65 exons
    many = [(2 * i, 2 * i, 20_000 + 50 * i, 20_000 + 50 * i + 9) for i in range(65)]
    est = bytes(gen[20_000:20_130])
    assert not GL.einval(len(est), glen, many, [_query(est, many)])
    assert GL.gaps(est, gen, many) == refused + (many, [0] * 65)
    got = GL.gaps(est, gen, many[:64])
    assert got[0] == GL.OK and len(got[5]) == 64 and all(1 <= s & 0x7F <= 2 for s in got[5][1:])
    # an EST gap of 64 / 65 bytes
    for gap, status in ((64, GL.OK), (65, GL.ERANGE)):
        e = bytes(gen[30_000:30_020]) + bytes(gen[30_020:30_020 + gap]) + bytes(gen[30_400:30_420])
        ex = [(0, 19, 30_000, 30_019), (20 + gap, 39 + gap, 30_400, 30_419)]
        assert not GL.einval(len(e), glen, ex, [_query(e, ex)])
        got = GL.gaps(e, gen, ex)
        assert got[0] == status
        if status == GL.ERANGE:
            assert got == refused + (ex, [0, 0])
        else:
            (ds, de, dgs, dge), (as_, ae, ags, age) = got[4]                      # the gap is the intron's first bytes: no error
            assert got[1:3] == (0, 0) and got[5] == [0, 1] and as_ == de + 1 and de - 19 == dge - 30_019 >= gap - 1
    # gapP == gapT against gapP == gapT + 1; EST_end == the next EST_start; GEN_end == the next GEN_start
    e = bytes(gen[30_000:30_050])
    for ex, bad in (([(0, 19, 30_000, 30_019), (30, 49, 30_030, 30_049)], False),          # 10 over 10
                    ([(0, 19, 30_000, 30_019), (30, 49, 30_029, 30_049)], True),           # 10 over 9
                    ([(0, 19, 30_000, 30_019), (20, 49, 30_020, 30_049)], False),          # 0 over 0
                    ([(0, 19, 30_000, 30_019), (20, 49, 30_019, 30_049)], True),           # GEN_end == GEN_start
                    ([(0, 19, 30_000, 30_019), (19, 49, 30_030, 30_049)], True),           # EST_end == EST_start
                    ([(0, 19, 30_000, 30_019), (18, 49, 30_030, 30_049)], True),
                    ([(0, 19, 30_000, 30_019), (20, 49, 30_018, 30_049)], True)):
        assert GL.einval(len(e), glen, ex, [_query(e, ex)]) == bad, ex
    got = GL.gaps(e, gen, [(0, 19, 30_000, 30_019), (30, 49, 30_030, 30_049)])               # p == t: distance 0, then merged
    assert got[:4] == (GL.OK, 0, 0, 1) and got[5] == [0, 1 | GL.MERGED] and got[4][0] == (0, 49, 30_000, 30_049)
    cut = got[4][1][0] - 20                                 # every cut costs nothing: wherever it fell, the gap closed
    assert 0 <= cut <= 10 and got[4][1] == (20 + cut, 49, 30_020 + cut, 30_049)
    # each bad query field
    c = next(c for c in cases if len(c["exons"]) >= 3)
    est, ex = c["est"], c["exons"]
    assert not GL.einval(len(est), glen, ex, [_query(est, ex)])
    for bad in (_query(est, ex, n_exons=0), _query(est, ex, n_exons=len(ex) + 1), _query(est, ex, first_exon=1),
                _query(est, ex, first_exon=len(ex) + 1, n_exons=1), _query(est, ex, est_len=len(est) + 1), _query(est, ex, est_off=1),
                _query(est, ex, reserved=1), _query(est, ex, est_len=0)):
        assert GL.einval(len(est), glen, ex, [bad]), bad
    assert GL.einval(1 << 32, glen, ex, [_query(est, ex, est_len=1 << 31)])                # inside its buffer, and too long
    assert not GL.einval(1 << 32, glen, ex, [_query(est, ex, est_len=(1 << 31) - 1)])
    assert GL.einval(len(est), glen, ex, [_query(est, ex, n_exons=2), _query(est, ex, first_exon=1, n_exons=len(ex) - 1)])
    assert not GL.einval(len(est), glen, ex, [_query(est, ex, n_exons=2), _query(est, ex, first_exon=2, n_exons=len(ex) - 2)])
    for k, v in ((0, -2), (1, len(est) + 1), (2, -2), (3, glen + 1)):
        e2 = list(ex)
        e2[1] = tuple(v if i == k else x for i, x in enumerate(ex[1]))
        assert GL.einval(len(est), glen, e2, [_query(est, ex)])
    # one exon, whatever its ends: nothing to compare them with
    assert not GL.einval(len(est), glen, [(-1, -1, -1, -1)], [_query(est, ex[:1])])
    assert GL.gaps(est, gen, [(5, 2, 9, 3)]) == (GL.OK, 0, 0, 1, [(5, 2, 9, 3)], [0])


def test_binding_matches_the_header():
    from pintron_amd import capi
    assert "pgpu_index_gap_chains" in capi.EXPORTS and "pgpu_index_gap_chains_kernel_ms" in capi.EXPORTS
    L = capi.lib()
    assert hasattr(L, "pgpu_index_gap_chains") and hasattr(L, "pgpu_index_gap_chains_kernel_ms")
    assert L.pgpu_abi_version() == 1
    text = open(BL.HEADER).read()
    assert int(re.search(r"#define PGPU_GAPS_MAX_EXONS\s+(\d+)", text).group(1)) == capi.GAPS_MAX_EXONS == GL.MAX_EXONS == 64
    assert int(re.search(r"#define PGPU_GAPS_MAX_EST_GAP\s+(\d+)", text).group(1)) == capi.GAPS_MAX_EST_GAP == GL.MAX_EST_GAP == 64
    assert int(re.search(r"#define PGPU_GAPS_MAX_ERRORS\s+(\d+)", text).group(1)) == capi.GAPS_MAX_ERRORS == GL.MAX_ERRORS == 20
    for cname, struct, dtype in (("pgpu_gaps_query", capi.GapsQuery, capi.GAPS_QUERY_DTYPE),
                                 ("pgpu_gaps_result", capi.GapsResult, capi.GAPS_RESULT_DTYPE)):
        BL.assert_layout(cname, struct, dtype)
    assert np.dtype(capi.FACTOR_DTYPE).itemsize == C.sizeof(capi.Factor) == 16


def test_host_side_of_the_entry_under_sanitizers(tmp_path):
    hipcc = resource_lib.hipcc()
    if not hipcc:
        pytest.skip("no ROCm headers here")
    include = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "include")
    exe = str(tmp_path / "gaps_call_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-D__HIP_PLATFORM_AMD__", "-I" + include, "-o", exe,
                    os.path.join(HERE, "hostcheck", "gaps_call_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout == "ok\n", (r.stdout, r.stderr[-2000:])
