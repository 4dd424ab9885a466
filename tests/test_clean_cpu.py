"""CPU: the restatement of pgpu_index_clean_chains (tests/clean_lib.py) against what the reference's six cleaning routines
left (tests/golden/clean_chains.json.gz), the cover of that fixture, the cap and PGPU_EINVAL rules of the restatement, and
the binding's layout against the header."""
import ctypes as C
import os
import re

import numpy as np

import binding_lib as BL
import clean_lib as CL
import refine_lib as RL

HEADER = BL.HEADER


def test_restatement_equals_the_fixture_on_every_case():
    gen, cases = CL.load_fixture()
    for k, c in enumerate(cases):
        info = {}
        got = CL.clean(c["est"], gen, c["exons"], c["thr"], info=info)
        assert got == (CL.OK, c["verdict"], c["first"], c["n"], c["exons_after"], c["marks"]), (k, got, c)
        assert set(CL.tags_of(info)) == c["tags"], (k, info, c["tags"])
        assert (c["n"] > 0) == (c["verdict"] in (0, 7))


def test_the_fixture_covers_what_it_must():
    gen, cases = CL.load_fixture()
    assert len(cases) >= 1000
    verdicts = [0] * 8
    tags = {t: 0 for t in ("head_trimmed", "tail_trimmed_gap", "single", "head_dropped_of_two", "tie", "band", "odd")}
    marks = [0] * 5
    for c in cases:
        verdicts[c["verdict"]] += 1
        for t in tags:
            tags[t] += t in c["tags"]
        for b in range(5):
            marks[b] += any(m >> b & 1 for m in c["marks"])
        assert 1 <= len(c["exons"]) <= 6
    assert min(verdicts) >= 25, verdicts
    assert min(tags.values()) >= 25, tags
    assert min(marks) >= 25, marks
    assert os.path.getsize(CL.FIXTURE) <= os.path.getsize(RL.FIXTURE)


def _query(est, ex, **kw):
    d = dict(est_off=0, est_len=len(est), first_exon=0, n_exons=len(ex), reserved=0, complexity_threshold=20.0)
    d.update(kw)
    return d


def test_caps_and_einval_rules_of_the_restatement():
    gen, cases = CL.load_fixture()
    c = next(c for c in cases if c["verdict"] == 0 and len(c["exons"]) >= 3 and c["exons"][0][0] > 0)
    est, ex = c["est"], c["exons"]
    refused = (CL.ERANGE, 0, 0, 0)
    # more than 64 exons, before any step looks at them
    many = [(i, i, 100 + 3 * i, 100 + 3 * i) for i in range(65)]
    assert CL.clean(b"A" * 65, gen, many, 20.0)[:4] == refused
    assert CL.clean(b"A" * 65, gen, many[:64], 20.0)[0] == CL.OK
    assert CL.clean(b"A" * 65, gen, many[::-1], 20.0)[:4] == refused              # (64 of them: verdict 2)
    assert CL.clean(b"A" * 65, gen, many[:64][::-1], 20.0)[:2] == (CL.OK, 2)
    # an end exon longer than 4096 on either string; 4096 is taken
    # (an exon of that length would meet the cap of step 5: the threshold lets step 4 reject it first)
    g = gen[1000:1000 + 4097]
    low = 1e-9
    assert CL.clean(g, gen, [(0, 4096, 1000, 5096)], low) == (CL.ERANGE, 0, 0, 0, [(0, 4096, 1000, 5096)], [0])
    assert CL.clean(g, gen, [(0, 4095, 1000, 5095)], low)[:2] == (CL.OK, 5)
    assert CL.clean(g, gen, [(0, 4095, 1000, 5096)], low)[0] == CL.ERANGE
    assert CL.clean(g, gen, [(0, 4095, 1000, 5095)], 20.0)[0] == CL.ERANGE        # step 5: a bound of 123
    # above 64 EST bytes the lengths must be within the band and the band must settle the score
    assert CL.clean(g, gen, [(0, 64, 1000, 1000 + 64 + 31)], 20.0)[0] == CL.OK
    assert CL.clean(g, gen, [(0, 64, 1000, 1000 + 64 + 32)], 20.0)[0] == CL.ERANGE
    assert CL.clean(g, gen, [(0, 63, 1000, 1000 + 63 + 32)], 20.0)[0] == CL.OK   # 64 EST bytes: lev_wave<ALIGN>
    # an earlier rejection never reaches a later cap: one exon that begins outside the EST, however long
    assert CL.clean(g, gen, [(-1, 4096, 1000, 5096)], 20.0)[:2] == (CL.OK, 1)
    # a bound beyond 31 at step 5: a genomic length of 1 034
    assert CL.max_edit(1033) == 31 and CL.max_edit(1034) == 32
    for glen, status in ((1033, CL.OK), (1034, CL.ERANGE)):
        e = gen[3000:3100] + gen[4000:4000 + glen] + gen[6000:6100]
        three = [(0, 99, 3000, 3099), (100, 100 + glen - 1, 4000, 4000 + glen - 1), (100 + glen, 199 + glen, 6000, 6099)]
        assert CL.clean(e, gen, three, 20.0)[0] == status
    # PGPU_EINVAL
    assert not CL.einval(len(est), len(gen), ex, [_query(est, ex)])
    for bad in (_query(est, ex, n_exons=0), _query(est, ex, n_exons=len(ex) + 1), _query(est, ex, first_exon=1),
                _query(est, ex, est_len=len(est) + 1), _query(est, ex, est_off=1), _query(est, ex, reserved=1),
                _query(est, ex, est_len=0)):
        assert CL.einval(len(est), len(gen), ex, [bad]), bad
    assert CL.einval(1 << 32, len(gen), ex, [_query(est, ex, est_len=1 << 31)])           # inside its buffer, and too long
    assert not CL.einval(1 << 32, len(gen), ex, [_query(est, ex, est_len=(1 << 31) - 1)])
    assert CL.einval(len(est), len(gen), ex, [_query(est, ex, n_exons=2), _query(est, ex, first_exon=1, n_exons=len(ex) - 1)])
    for k, v in ((0, -2), (1, len(est) + 1), (2, -2), (3, len(gen) + 1)):
        e2 = list(ex)
        e2[1] = tuple(v if i == k else x for i, x in enumerate(ex[1]))
        assert CL.einval(len(est), len(gen), e2, [_query(est, ex)])
    # the my_asserts of handle_endpoints, for a query that passes the two checks
    for place, k, v in ((0, 0, -1), (0, 2, -1), (-1, 1, len(est)), (-1, 3, len(gen))):
        e2 = list(ex)
        e2[place] = tuple(v if i == k else x for i, x in enumerate(ex[place]))
        assert CL.passes_step1(e2, len(est)) and CL.einval(len(est), len(gen), e2, [_query(est, ex)]), (place, k)
    # ... and not for one that does not: one exon that begins outside the EST is verdict 1
    assert not CL.einval(len(est), len(gen), [(-1, 5, 100, 106)], [_query(est, ex[:1])])
    assert not CL.einval(len(est), len(gen), [(len(est), len(est), 100, 106)], [_query(est, ex[:1])])
    assert not CL.einval(len(est), len(gen), [(53, -1, 100, 106)], [_query(est, ex[:1])])         # one exon, reversed: verdict 2
    e2 = [ex[1], ex[0]] + list(ex[2:])                                            # out of order: verdict 2
    assert not CL.einval(len(est), len(gen), e2, [_query(est, ex)])


def test_binding_matches_the_header():
    from pintron_amd import capi
    assert "pgpu_index_clean_chains" in capi.EXPORTS and "pgpu_index_clean_chains_kernel_ms" in capi.EXPORTS
    L = capi.lib()
    assert hasattr(L, "pgpu_index_clean_chains") and hasattr(L, "pgpu_index_clean_chains_kernel_ms")
    assert L.pgpu_abi_version() == 1
    text = open(HEADER).read()
    assert int(re.search(r"#define PGPU_CLEAN_MAX_EXONS\s+(\d+)", text).group(1)) == capi.CLEAN_MAX_EXONS == CL.MAX_EXONS == 64
    assert int(re.search(r"#define PGPU_CLEAN_MAX_END_EXON\s+(\d+)", text).group(1)) == capi.CLEAN_MAX_END_EXON == CL.MAX_END_EXON == 4096
    band = open(os.path.join(RL.ROOT, "pintron_amd", "csrc", "pgpu_internal.h")).read()
    assert int(re.search(r"constexpr uint32_t ALIGN_BAND_HALF = (\d+)u;", band).group(1)) == CL.BAND_HALF == CL.MAX_KBAND
    for cname, struct, dtype in (("pgpu_clean_query", capi.CleanQuery, capi.CLEAN_QUERY_DTYPE),
                                 ("pgpu_clean_result", capi.CleanResult, capi.CLEAN_RESULT_DTYPE)):
        BL.assert_layout(cname, struct, dtype)
    assert np.dtype(capi.FACTOR_DTYPE).itemsize == C.sizeof(capi.Factor) == 16
