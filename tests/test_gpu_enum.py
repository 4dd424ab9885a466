"""GPU: the enumeration stage -- pgpu_index_candidate_lists against the fixture tests/golden/candidate_lists.json.gz, the
hand-made records in every company, the entry's refusals, the cap edges and the cyclic records between answered
neighbours, the plan form (run -> run_meg -> run_candidate_lists, nothing of a record leaving HBM) against the restatement
(tests/enum_lib.py) on the device's own fetched records, against the index form and against the candidate stage, the rule
of the branch beside the stages, and one use of the output by pgpu_index_clean_chains.  Every comparison is byte equality."""
import ctypes as C

import numpy as np
import pytest

import cand_lib as CL
import enum_lib as EL
import meg_lib as M

pytestmark = pytest.mark.gpu

BAD_RECORD = ("bad MEG record (offsets not ascending, past the buffer or not at a multiple of 4, a record shorter than its "
              "counts need, more than 64 vertices, CSR offsets out of order or past n_edges, a target that is no vertex, or a "
              "vertex outside what it indexes)")
BAD_PARAMS = "bad candidate parameters (min_factor_len 0 or above 2^24)"
NAMES = ("results", "candidates", "exons")


def same(got, want, what=""):
    for name, g, w in zip(NAMES, got, want):
        assert len(g) == len(w), (what, name, len(g), len(w))
        if g.tobytes() != w.tobytes():
            bad = [i for i in range(len(g)) if g[i] != w[i]]
            raise AssertionError("%s: %s differ at %d places, first %d: %r / %r" % (what, name, len(bad), bad[0], g[bad[0]], w[bad[0]]))


@pytest.fixture(scope="module")
def golden(gpu_ctx):
    """the fixture, grouped: {(sequence, L, min_intron): [case]}, and one index per sequence"""
    import pintron_amd.capi as capi
    seqs, cases, _ = EL.load_fixture()
    groups = {}
    for c in cases:
        groups.setdefault((c["seq"], c["L"], c["min_intron"]), []).append(c)
    idx = {name: capi.Index(gpu_ctx, g) for name, g in seqs.items()}
    yield seqs, groups, idx
    for i in idx.values():
        i.close()


def wanted(cases):
    return EL.expect_arrays([EL.answer_of(c) for c in cases])


def test_every_golden_case_one_call_per_parameter_pair_and_again(golden):
    seqs, groups, idx = golden
    assert sum(len(g) for g in groups.values()) > 1200
    for (seq, L, mi), cases in groups.items():
        recs = [c["record"] for c in cases]
        first = idx[seq].candidate_lists(recs, L, mi)
        same(first, wanted(cases), (seq, L, mi))
        assert idx[seq].candidate_lists_kernel_ms() > 0.0     # the fixture's context has timing on
        again = idx[seq].candidate_lists(recs, L, mi)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(first, again))


def test_golden_cases_on_a_loaded_index(golden, gpu_ctx, tmp_path):
    import pintron_amd.capi as capi
    seqs, groups, idx = golden
    for seq in ("hand", "issue13"):
        path = str(tmp_path / (seq + ".idx"))
        idx[seq].save(path)
        loaded = capi.Index(gpu_ctx, seqs[seq], load_from=path)
        try:
            for (s, L, mi), cases in groups.items():
                if s == seq:
                    same(loaded.candidate_lists([c["record"] for c in cases], L, mi), wanted(cases), (seq, L, mi))
        finally:
            loaded.close()


def hand(golden):
    seqs, groups, idxs = golden
    cases = [c for c in groups[("hand", 15, 40)] if c["name"].startswith("hand/")]
    return seqs["hand"], idxs["hand"], cases, {c["name"][len("hand/"):]: c for c in cases}


def test_hand_made_records_in_every_company(golden):
    g, idx, cases, _ = hand(golden)
    assert len(cases) > 60
    recs = [c["record"] for c in cases]
    same(idx.candidate_lists(recs, 15, 40), wanted(cases), "one batch")
    same(idx.candidate_lists(recs[::-1], 15, 40), wanted(cases[::-1]), "reversed")
    for c in cases:                                            # an answer never depends on its neighbours
        same(idx.candidate_lists([c["record"]], 15, 40), wanted([c]), c["name"])


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65])
def test_batch_sizes(golden, n):
    g, idx, cases, by_name = hand(golden)
    pick = [cases[(7 * k) % len(cases)] for k in range(n)]
    if n:
        pick[-1] = by_name["degree_32_1"]                       # the last record has work to do
    same(idx.candidate_lists([c["record"] for c in pick], 15, 40), wanted(pick), n)


def test_cap_edges_and_cyclic_records_between_answered_neighbours(golden):
    g, idx, cases, by_name = hand(golden)
    fill = [by_name[n] for n in ("equal_2_0", "diamond_1", "second_root_2", "degree_32_0", "vertices_64_1", "longer_2_2")]
    batch = []
    for k, name in enumerate(("list_64", "list_65", "embeddings_512", "embeddings_513", "list_80", "cycle", "self_loop", "cycle_unreached")):
        batch += [fill[k % len(fill)], by_name[name]]
    batch.append(fill[0])
    res, cands, exons = idx.candidate_lists([c["record"] for c in batch], 15, 40)
    same((res, cands, exons), wanted(batch))
    kinds = {c["name"][len("hand/"):]: (int(r["kind"]), int(r["detail"])) for c, r in zip(batch, res)}
    assert kinds["list_64"] == (EL.LISTS, 0) and kinds["list_65"] == (EL.RANGE, EL.CAP_LIST) and kinds["list_80"] == (EL.RANGE, EL.CAP_LIST)
    assert kinds["embeddings_512"] == (EL.LISTS, 0) and kinds["embeddings_513"] == (EL.RANGE, EL.CAP_EMBEDDINGS)
    assert kinds["cycle"] == kinds["self_loop"] == kinds["cycle_unreached"] == (EL.CYCLIC, 0)
    assert all(int(r["kind"]) == EL.LISTS and int(r["n_candidates"]) > 0 for r in res[::2])       # every neighbour is answered
    assert int(res[1]["n_candidates"]) == 64


def test_refusals_and_the_contract_of_the_index_form(golden, gpu_ctx):
    import pintron_amd.capi as capi
    L_ = gpu_ctx.L
    g, idx, cases, by_name = hand(golden)
    glen = len(g)
    cases = cases[:40]
    recs = [c["record"] for c in cases]
    want = wanted(cases)
    n_c, n_e = len(want[1]), len(want[2])
    assert n_c > 20 and n_e > n_c
    blob, first = CL.batch(recs)
    f = L_.pgpu_index_candidate_lists

    def raw(blob_, first_, n, L=15, mi=40, ccap=None, ecap=None, blob_len=None):
        ccap, ecap = n_c if ccap is None else ccap, n_e if ecap is None else ecap
        res = np.full(16 * max(n, 1), 0x55, dtype=np.uint8).view(np.dtype(capi.ENUM_RESULT_DTYPE))
        cd = np.full(16 * max(ccap, 1), 0x55, dtype=np.uint8).view(np.dtype(capi.ENUM_CANDIDATE_DTYPE))
        ex = np.full(16 * max(ecap, 1), 0x55, dtype=np.uint8).view(np.dtype(capi.FACTOR_DTYPE))
        nc, ne = C.c_size_t(12345), C.c_size_t(54321)
        prm = capi.CandParams(L, mi)
        rc = f(gpu_ctx.h, idx.h, blob_, len(blob_) if blob_len is None else blob_len, first_.ctypes.data_as(C.POINTER(C.c_uint64)), n,
               C.byref(prm), res.ctypes.data_as(C.POINTER(capi.EnumResult)), cd.ctypes.data_as(C.POINTER(capi.EnumCandidate)), ccap,
               ex.ctypes.data_as(C.POINTER(capi.Factor)), ecap, C.byref(nc), C.byref(ne))
        untouched = all((x.view(np.uint8) == 0x55).all() for x in (res, cd, ex))
        return rc, untouched, (nc.value, ne.value), (res, cd, ex)

    def good():
        rc, _, counts, (res, cd, ex) = raw(blob, first, len(recs))
        assert rc == capi.PGPU_OK and counts == (n_c, n_e)
        same((res, cd[:n_c], ex[:n_e]), want)
        assert idx.candidate_lists_kernel_ms() > 0.0

    def refused(blob_, first_, n, message=BAD_RECORD, **kw):
        good()                                                                   # a slot for the refusal to reset
        rc, untouched, counts, _ = raw(blob_, first_, n, **kw)
        assert rc == capi.PGPU_EINVAL and untouched and counts == (12345, 54321)
        assert CL.einval(blob_[:kw.get("blob_len", len(blob_))], first_, glen, kw.get("L", 15))
        assert L_.pgpu_last_error(gpu_ctx.h).decode() == message and idx.candidate_lists_kernel_ms() == 0.0

    refused(blob, first, len(recs), message=BAD_PARAMS, L=0)
    refused(blob, first, len(recs), message=BAD_PARAMS, L=(1 << 24) + 1)
    refused(blob, first, len(recs), blob_len=len(blob) - 4)                      # the last record runs past the buffer
    for k, value in ((3, int(first[2]) - 4), (len(recs), len(blob) + 4), (5, int(first[5]) + 2)):
        o = first.copy()
        o[k] = value
        refused(blob, o, len(recs))
    # one malformed record in the middle of the batch: each way the header lists (the validator is pgpu_index_candidates')
    base = CL.record(*CL.chain([(100, 2000, 40), (140, 2200, 40)]))
    v, a = CL.chain([(100, 2000, 40), (140, 2200, 40)])
    bad = [base[:76], base[:12],
           CL.record([CL.SOURCE] + [(k, k, 1) for k in range(63)] + [CL.SINK], [[k + 1] for k in range(64)] + [[]]),      # 65 vertices
           CL.record(v, a, n_edges=2), CL.record(v, a, n_edges=1 << 20),
           CL.record(v, [[1], [2], [4], []]), CL.record(v, [[1], [2], [255], []]),
           CL.record([v[0], (100, glen - 39, 40)] + v[2:], a), CL.record([v[0], (100, -1, 40)] + v[2:], a),
           CL.record([v[0], (100, 2000, -1)] + v[2:], a), CL.record([v[0], (-1, 2000, 40)] + v[2:], a),
           CL.record([v[0], ((1 << 29) - 39, 2000, 40)] + v[2:], a),
           CL.record([(CL.SOURCE_P, 0, 200)] + v[1:], a), CL.record(v[:-1] + [(CL.SINK_P, CL.SINK_P, 199)], a)]
    csr_bad = bytearray(base)
    csr_bad[16 + 48 + 4:16 + 48 + 6] = (0).to_bytes(2, "little")                   # first[2] < first[1]
    bad.append(bytes(csr_bad))
    for k, r in enumerate(bad):
        assert CL.record_einval(r, glen) and len(r) % 4 == 0, k
        b2, f2 = CL.batch(recs[:7] + [r] + recs[7:])
        refused(b2, f2, len(recs) + 1)
    shifted = first.copy()                                                        # a record that is not at a multiple of 4
    shifted[1:] += 2
    refused(blob[:int(first[1])] + b"\0\0" + blob[int(first[1]):], shifted, len(recs))
    # PGPU_ENOSPC, both shapes: both counts, and nothing written
    for ccap, ecap in ((0, n_e), (n_c - 1, n_e), (n_c, 0), (n_c, n_e - 1), (0, 0)):
        good()
        rc, untouched, counts, _ = raw(blob, first, len(recs), ccap=ccap, ecap=ecap)
        assert rc == capi.PGPU_ENOSPC and untouched and counts == (n_c, n_e) and idx.candidate_lists_kernel_ms() == 0.0
        assert ("candidate" if ccap < n_c else "exon") in L_.pgpu_last_error(gpu_ctx.h).decode()
    # null pointers: a bare refusal, the message stays
    good()
    raw(blob, first, len(recs), L=0)
    res = np.zeros(len(recs), dtype=np.dtype(capi.ENUM_RESULT_DTYPE))
    cd = np.zeros(n_c, dtype=np.dtype(capi.ENUM_CANDIDATE_DTYPE))
    ex = np.zeros(n_e, dtype=np.dtype(capi.FACTOR_DTYPE))
    nc, ne = C.c_size_t(0), C.c_size_t(0)
    prm = capi.CandParams(15, 40)
    fp, rp = first.ctypes.data_as(C.POINTER(C.c_uint64)), res.ctypes.data_as(C.POINTER(capi.EnumResult))
    cp, ep = cd.ctypes.data_as(C.POINTER(capi.EnumCandidate)), ex.ctypes.data_as(C.POINTER(capi.Factor))
    full = [gpu_ctx.h, idx.h, blob, len(blob), fp, len(recs), C.byref(prm), rp, cp, n_c, ep, n_e, C.byref(nc), C.byref(ne)]
    for k in (0, 1, 2, 4, 6, 7, 8, 10, 12, 13):
        args = list(full)
        args[k] = None
        assert f(*args) == capi.PGPU_EINVAL, k
        if k:
            assert L_.pgpu_last_error(gpu_ctx.h).decode() == BAD_PARAMS and idx.candidate_lists_kernel_ms() == 0.0
    # n == 0
    good()
    nc.value = ne.value = 99
    assert f(gpu_ctx.h, idx.h, None, 0, None, 0, C.byref(prm), None, None, 0, None, 0, C.byref(nc), C.byref(ne)) == capi.PGPU_OK
    assert (nc.value, ne.value) == (0, 0) and idx.candidate_lists_kernel_ms() == 0.0
    # a batch without a candidate: no buffer needed
    nc.value = ne.value = 99
    none = [CL.bare(CL.UNAVAILABLE), by_name["cycle"]["record"], by_name["no_vertex"]["record"], by_name["list_65"]["record"]]
    b0, f0 = CL.batch(none)
    assert f(gpu_ctx.h, idx.h, b0, len(b0), f0.ctypes.data_as(C.POINTER(C.c_uint64)), 4, C.byref(prm), rp, None, 0, None, 0,
             C.byref(nc), C.byref(ne)) == capi.PGPU_OK
    assert (nc.value, ne.value) == (0, 0) and list(res["kind"][:4]) == [EL.NONE, EL.CYCLIC, EL.LISTS, EL.RANGE]
    good()                                                                       # the context still answers


def test_without_timing_the_answers_are_the_same(golden):
    import pintron_amd.capi as capi
    g, _, cases, _ = hand(golden)
    recs = [c["record"] for c in cases]
    with capi.Context(0) as ctx:
        idx = capi.Index(ctx, g)
        same(idx.candidate_lists(recs, 15, 40), wanted(cases))
        assert idx.candidate_lists_kernel_ms() > 0.0
        ctx.L.pgpu_set_timing(ctx.h, 0)
        same(idx.candidate_lists(recs, 15, 40), wanted(cases))
        assert idx.candidate_lists_kernel_ms() == 0.0
        idx.close()


# ---- the plan form ------------------------------------------------------------------------------------------------
def run_plan(plan, prm, rate=0.2, mi=None):
    plan.run(prm["min_factor_len"], rate)
    plan.run_meg(**prm)
    plan.run_candidate_lists(prm["min_factor_len"], prm["min_intron_length"] if mi is None else mi)
    return plan.fetch_candidate_lists()


@pytest.mark.parametrize("source,n_pat", [("c2", 307), ("issue13", 1891)])
@pytest.mark.parametrize("resident", [False, True])
def test_plan_form_against_the_restatement_the_index_form_and_the_candidate_stage(gpu_ctx, source, n_pat, resident):
    import pintron_amd.capi as capi
    gfa, efa = CL.real_inputs()[source]
    prm = M.DEFAULTS
    exp, genomic = M.first_attempt_megs(gfa, efa, prm)
    assert len(exp) == n_pat
    L, mi = prm["min_factor_len"], prm["min_intron_length"]
    idx = capi.Index(gpu_ctx, genomic)
    plan = capi.PairingPlan(gpu_ctx, idx, [e["seq"] for e in exp], resident=resident)
    try:
        got = run_plan(plan, prm)
        assert plan.candidate_lists_ms() > 0.0
        assert plan.candidate_list_counts() == (len(got[1]), len(got[2]))
        recs = plan.fetch_meg()
        # every pattern: the restatement on the device's own record
        mine = [EL.candidate_lists(r, genomic, L, mi) for r in recs]
        same(got, EL.expect_arrays(mine), source)
        kinds = np.bincount(got[0]["kind"], minlength=4)
        assert kinds[EL.LISTS] > n_pat // 2 and kinds[EL.CYCLIC] == 0, kinds
        assert max(len(m[4]) for m in mine) > 1
        # the index form on the fetched records: byte for byte
        same(idx.candidate_lists(recs, L, mi), got, source + " index form")
        # the candidate stage, on every pattern it calls ONE or REFUSED
        plan.run_candidates(L, mi)
        cres, cex = plan.fetch_candidates()
        n_one = 0
        answers = EL.answers_of_arrays(*got)
        for k in range(n_pat):
            kind = int(cres["kind"][k])
            if kind not in (CL.ONE, CL.REFUSED):
                continue
            a = answers[k]
            assert a[:4] == (EL.LISTS, 0, int(cres["work"][k]), 1), (source, k)
            if kind == CL.ONE:
                at, n = int(cres["first_exon"][k]), int(cres["n_exons"][k])
                assert a[4] == [(0, int(cres["n_pairs"][k]), [tuple(int(x) for x in e) for e in cex[at:at + n].tolist()])], (source, k)
                n_one += 1
            else:
                assert a[4] == [], (source, k)
        assert n_one > n_pat // 3
        # run_candidates left the lists fetchable and unchanged
        same(plan.fetch_candidate_lists(), got, source + " behind run_candidates")
        # a rerun, other parameters and back: the same bytes
        again = run_plan(plan, prm)
        got0 = run_plan(plan, M.params(min_intron_length=0))
        same(got0, EL.expect_arrays([EL.candidate_lists(r, genomic, L, 0) for r in plan.fetch_meg()]), source + " intron0")
        back = run_plan(plan, prm)
        for g in (again, back):
            assert all(x.tobytes() == y.tobytes() for x, y in zip(g, got))
        # min_intron_length is the stage's own: the same records under another value
        plan.run_candidate_lists(L, 200)
        same(plan.fetch_candidate_lists(), EL.expect_arrays([EL.candidate_lists(r, genomic, L, 200) for r in recs]), source + " 200")
    finally:
        plan.close()
        idx.close()


def test_the_branch_rule_and_the_refusals_of_the_plan_form(gpu_ctx):
    import pintron_amd.capi as capi
    L_ = gpu_ctx.L
    gfa, efa = M.rerun_input()
    exp, genomic = M.first_attempt_megs(gfa, efa)
    seqs = [e["seq"] for e in exp]
    idx = capi.Index(gpu_ctx, genomic)
    plan = capi.PairingPlan(gpu_ctx, idx, seqs)
    res = np.zeros(len(seqs), dtype=np.dtype(capi.ENUM_RESULT_DTYPE))
    cd = np.zeros(1 << 14, dtype=np.dtype(capi.ENUM_CANDIDATE_DTYPE))
    ex = np.zeros(1 << 16, dtype=np.dtype(capi.FACTOR_DTYPE))
    rp, cp, ep = (res.ctypes.data_as(C.POINTER(capi.EnumResult)), cd.ctypes.data_as(C.POINTER(capi.EnumCandidate)),
                  ex.ctypes.data_as(C.POINTER(capi.Factor)))

    def run_l(L, mi=40, p=None):
        prm = capi.CandParams(L, mi)
        return L_.pgpu_pairing_plan_run_candidate_lists(gpu_ctx.h, (p or plan).h, C.byref(prm))

    def fetch(ccap=1 << 14, ecap=1 << 16, p=None):
        return L_.pgpu_pairing_plan_fetch_candidate_lists(gpu_ctx.h, (p or plan).h, rp, cp, ccap, ep, ecap)

    def message():
        return L_.pgpu_last_error(gpu_ctx.h).decode()

    def blob(arrays):
        return [np.asarray(a).tobytes() for a in arrays]
    try:
        assert fetch() == capi.PGPU_EINVAL and "run_candidate_lists" in message()          # nothing ran yet
        assert run_l(15) == capi.PGPU_EINVAL and "run_meg" in message()
        plan.run(15, 0.2)
        assert run_l(15) == capi.PGPU_EINVAL and "run_meg" in message()                      # pairings, no records
        plan.run_meg(**M.DEFAULTS)
        assert run_l(0) == capi.PGPU_EINVAL and message() == BAD_PARAMS
        assert run_l((1 << 24) + 1) == capi.PGPU_EINVAL and message() == BAD_PARAMS
        assert run_l(16) == capi.PGPU_EINVAL and "same min_factor_len" in message()
        assert fetch() == capi.PGPU_EINVAL and plan.candidate_list_counts() == (0, 0) and plan.candidate_lists_ms() == 0.0
        # the ladder is climbed first; the branch leaves every rung fetchable and unchanged
        plan.run_candidates(15, 40)
        plan.run_factorizations()
        before = blob(plan.fetch_candidates()) + blob(plan.fetch_factorizations()) + blob([b"".join(plan.fetch_meg())])
        assert run_l(15) == capi.PGPU_OK
        n_c, n_e = plan.candidate_list_counts()
        assert n_c > 0 and n_e >= n_c and plan.candidate_lists_ms() > 0.0
        after = blob(plan.fetch_candidates()) + blob(plan.fetch_factorizations()) + blob([b"".join(plan.fetch_meg())])
        assert before == after
        assert fetch(n_c - 1, n_e) == capi.PGPU_ENOSPC and fetch(n_c, n_e - 1) == capi.PGPU_ENOSPC and fetch(0, 0) == capi.PGPU_ENOSPC
        assert fetch(n_c, n_e) == capi.PGPU_OK
        want = (res.copy(), cd[:n_c].copy(), ex[:n_e].copy())
        same(want, EL.expect_arrays([EL.candidate_lists(r, genomic, 15, 40) for r in plan.fetch_meg()]))
        # the rungs above the records neither need the branch nor disturb it
        plan.run_candidates(15, 40)
        plan.run_factorizations()
        plan.run_final_factorizations()
        assert fetch(n_c, n_e) == capi.PGPU_OK
        assert (res.tobytes(), cd[:n_c].tobytes(), ex[:n_e].tobytes()) == tuple(w.tobytes() for w in want)
        # null pointers
        assert L_.pgpu_pairing_plan_run_candidate_lists(gpu_ctx.h, plan.h, None) == capi.PGPU_EINVAL
        assert fetch(n_c, n_e) == capi.PGPU_OK                                            # (a null pointer touches nothing)
        assert run_l(16) == capi.PGPU_EINVAL and fetch(n_c, n_e) == capi.PGPU_EINVAL         # a refused run took its results along
        assert run_l(15) == capi.PGPU_OK and fetch(n_c, n_e) == capi.PGPU_OK
        assert (res.tobytes(), cd[:n_c].tobytes(), ex[:n_e].tobytes()) == tuple(w.tobytes() for w in want)
        assert L_.pgpu_pairing_plan_run_candidate_lists(gpu_ctx.h, None, C.byref(capi.CandParams(15, 40))) == capi.PGPU_EINVAL
        assert L_.pgpu_pairing_plan_fetch_candidate_lists(gpu_ctx.h, plan.h, None, cp, n_c, ep, n_e) == capi.PGPU_EINVAL
        assert L_.pgpu_pairing_plan_candidate_list_counts(None, None, None) == capi.PGPU_EINVAL
        assert L_.pgpu_pairing_plan_candidate_lists_ms(None) == 0.0
        # run_meg and run end them
        plan.run_meg(**M.DEFAULTS)
        assert fetch(n_c, n_e) == capi.PGPU_EINVAL and "run_candidate_lists" in message()
        assert run_l(15) == capi.PGPU_OK and fetch(n_c, n_e) == capi.PGPU_OK
        plan.run(15, 0.2)
        assert fetch(n_c, n_e) == capi.PGPU_EINVAL and "run_candidate_lists" in message()
        assert run_l(15) == capi.PGPU_EINVAL and "run_meg" in message()
    finally:
        plan.close()
    # two resident plans: the one whose results the other's run overwrote
    a = capi.PairingPlan(gpu_ctx, idx, seqs[:30], resident=True)
    b = capi.PairingPlan(gpu_ctx, idx, seqs[30:], resident=True)
    try:
        for p in (a, b):
            p.run(15, 0.2)
            p.run_meg(**M.DEFAULTS)
            p.run_candidate_lists(15, 40)
        assert fetch(p=a) == capi.PGPU_EINVAL and "overwritten" in message()
        assert run_l(15, p=a) == capi.PGPU_EINVAL and "overwritten" in message()
        same(b.fetch_candidate_lists(), EL.expect_arrays([EL.candidate_lists(r, genomic, 15, 40) for r in b.fetch_meg()]))
        a.run(15, 0.2)
        a.run_meg(**M.DEFAULTS)
        a.run_candidate_lists(15, 40)
        same(a.fetch_candidate_lists(), EL.expect_arrays([EL.candidate_lists(r, genomic, 15, 40) for r in a.fetch_meg()]))
        assert fetch(p=b) == capi.PGPU_EINVAL and "overwritten" in message()
    finally:
        a.close()
        b.close()
        idx.close()


def test_empty_plan(gpu_ctx):
    import pintron_amd.capi as capi
    idx = capi.Index(gpu_ctx, b"ACGTTGCATGCATGCCGTA" * 20)
    for resident in (False, True):
        plan = capi.PairingPlan(gpu_ctx, idx, [], resident=resident)
        try:
            prm = capi.CandParams(15, 40)
            assert gpu_ctx.L.pgpu_pairing_plan_run_candidate_lists(gpu_ctx.h, plan.h, C.byref(prm)) == capi.PGPU_OK
            assert plan.candidate_list_counts() == (0, 0) and plan.candidate_lists_ms() == 0.0
            assert gpu_ctx.L.pgpu_pairing_plan_fetch_candidate_lists(gpu_ctx.h, plan.h, None, None, 0, None, 0) == capi.PGPU_OK
        finally:
            plan.close()
    idx.close()


# ---- one use of the output ----------------------------------------------------------------------------------------
def test_candidates_go_through_clean_chains_one_query_each(gpu_ctx):
    """the shape claim: a candidate's exons are a query of pgpu_index_clean_chains as they lie, the candidates of a record
    sharing their EST"""
    import clean_lib as KL
    import pintron_amd.capi as capi
    gfa, efa = CL.real_inputs()["issue13"]
    prm = M.DEFAULTS
    exp, genomic = M.first_attempt_megs(gfa, efa, prm)
    L, mi = prm["min_factor_len"], prm["min_intron_length"]
    idx = capi.Index(gpu_ctx, genomic)
    plan = capi.PairingPlan(gpu_ctx, idx, [e["seq"] for e in exp])
    try:
        res, cands, exons = run_plan(plan, prm)
        # three records with several candidates none of which is the source or the sink alone
        picked = []
        for k in np.argsort(-res["n_candidates"].astype(np.int64), kind="stable"):
            r = res[k]
            cs = cands[int(r["first_candidate"]):int(r["first_candidate"]) + int(r["n_candidates"])]
            ex = [exons[int(c["first_exon"]):int(c["first_exon"]) + int(c["n_exons"])] for c in cs]
            est = exp[int(k)]["seq"]
            if 2 <= len(cs) <= 8 and all(0 <= int(e["EST_start"][0]) and int(e["EST_end"][-1]) < len(est) for e in ex):
                picked.append((est, ex))
            if len(picked) == 3:
                break
        assert len(picked) == 3
        queries = [(est, [tuple(int(x) for x in e) for e in one.tolist()], 20.0) for est, ex in picked for one in ex]
        ests, ex_arr, q = KL.batch_arrays(queries)
        assert len(ests) == sum(len(est) for est, _ in picked)                  # the candidates of a record share their EST
        got = idx.clean_chains(ests, ex_arr, q)
        want = KL.expect_arrays(ex_arr, [KL.clean(est, genomic, ex, thr) for est, ex, thr in queries])
        for name, gx, wx in zip(("exons", "marks", "results"), got, want):
            assert gx.tobytes() == wx.tobytes(), name
        assert (got[2]["status"] == 0).all()
    finally:
        plan.close()
        idx.close()
