"""GPU: the candidate stage -- pgpu_index_candidates against the fixture whose Burset frequencies are the reference's, the
plan form (run -> run_meg -> run_candidates, nothing of a record leaving HBM) against the restatement (tests/cand_lib.py)
applied to the device's own fetched records and to the host's graphs, and the plan form against the index form.  Every
comparison is byte equality."""
import ctypes as C

import numpy as np
import pytest

import cand_lib as CL
import meg_lib as M

pytestmark = pytest.mark.gpu

BAD_RECORD = ("bad MEG record (offsets not ascending, past the buffer or not at a multiple of 4, a record shorter than its "
              "counts need, more than 64 vertices, CSR offsets out of order or past n_edges, a target that is no vertex, or a "
              "vertex outside what it indexes)")
BAD_PARAMS = "bad candidate parameters (min_factor_len 0 or above 2^24)"


def same(got, want, what=""):
    for name, g, w in (("results", got[0], want[0]), ("exons", got[1], want[1])):
        assert len(g) == len(w), (what, name, len(g), len(w))
        if g.tobytes() != w.tobytes():
            bad = [i for i in range(len(g)) if g[i] != w[i]]
            raise AssertionError("%s: %s differ at %d places, first %d: %r / %r" % (what, name, len(bad), bad[0], g[bad[0]], w[bad[0]]))


@pytest.fixture(scope="module")
def golden(gpu_ctx):
    """the fixture, grouped: {(sequence, L, min_intron): [case]}, and one index per sequence"""
    import pintron_amd.capi as capi
    seqs, cases = CL.load_fixture()
    groups = {}
    for c in cases:
        groups.setdefault((c["seq"], c["L"], c["min_intron"]), []).append(c)
    idx = {name: capi.Index(gpu_ctx, g) for name, g in seqs.items()}
    yield seqs, groups, idx
    for i in idx.values():
        i.close()


def answers(cases):
    return [(c["kind"], c["work"], c["n_pairs"], c["exons"]) for c in cases]


def test_every_golden_case_one_call_per_parameter_pair_and_again(golden):
    seqs, groups, idx = golden
    assert sum(len(g) for g in groups.values()) > 9000
    for (seq, L, mi), cases in groups.items():
        recs = [c["record"] for c in cases]
        want = CL.expect_arrays(answers(cases))
        first = idx[seq].candidates(recs, L, mi)
        same(first, want, (seq, L, mi))
        assert idx[seq].candidates_kernel_ms() > 0.0           # the fixture's context has timing on
        again = idx[seq].candidates(recs, L, mi)
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
                    same(loaded.candidates([c["record"] for c in cases], L, mi), CL.expect_arrays(answers(cases)), (seq, L, mi))
        finally:
            loaded.close()


# ---- the plan form ------------------------------------------------------------------------------------------------
def run_plan(plan, prm, rate=0.2):
    plan.run(prm["min_factor_len"], rate)
    plan.run_meg(**prm)
    plan.run_candidates(prm["min_factor_len"], prm["min_intron_length"])
    return plan.fetch_candidates()


@pytest.mark.parametrize("source,n_pat", [("c2", 307), ("issue13", 1891)])
@pytest.mark.parametrize("resident", [False, True])
def test_plan_form_against_the_restatement_the_host_graphs_and_the_index_form(gpu_ctx, source, n_pat, resident):
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
        assert plan.candidates_ms() > 0.0
        recs = plan.fetch_meg()
        # every pattern: the restatement on the device's own record, no record left out
        mine = [CL.candidate(r, genomic, L, mi) for r in recs]
        same(got, CL.expect_arrays(mine), source)
        kinds = np.bincount(got[0]["kind"], minlength=4)
        assert kinds[CL.ONE] > n_pat // 3 and kinds[CL.NOT_PATH] > 0, kinds
        # where the device had to build the graph: the restatement on the host's graph
        host_recs, _ = CL.host_records(gfa, efa, prm)
        n_avail = 0
        for k, e in enumerate(exp):
            if M.availability(e["stats"], prm) == "available":
                assert mine[k] == CL.candidate(host_recs[k], genomic, L, mi), (source, k)
                n_avail += 1
            flagged = bool(CL.parse(recs[k])[0] & 3)
            assert (got[0]["kind"][k] == CL.NONE) == flagged, (source, k)
        assert n_avail > n_pat // 2
        # the index form on the fetched records: byte for byte
        same(idx.candidates(recs, L, mi), got, source + " index form")
        # a rerun, other parameters and back: the same bytes
        again = run_plan(plan, prm)
        other = M.params(min_intron_length=0)
        got0 = run_plan(plan, other)
        same(got0, CL.expect_arrays([CL.candidate(r, genomic, L, 0) for r in plan.fetch_meg()]), source + " intron0")
        back = run_plan(plan, prm)
        for g in (again, back):
            assert g[0].tobytes() == got[0].tobytes() and g[1].tobytes() == got[1].tobytes()
        # min_intron_length is the candidate stage's own: the same records under another value
        plan.run_candidates(L, 200)
        same(plan.fetch_candidates(), CL.expect_arrays([CL.candidate(r, genomic, L, 200) for r in recs]), source + " 200")
    finally:
        plan.close()
        idx.close()


def test_refusals_of_the_plan_form(gpu_ctx):
    import pintron_amd.capi as capi
    L_ = gpu_ctx.L
    gfa, efa = M.rerun_input()
    exp, genomic = M.first_attempt_megs(gfa, efa)
    seqs = [e["seq"] for e in exp]
    idx = capi.Index(gpu_ctx, genomic)
    plan = capi.PairingPlan(gpu_ctx, idx, seqs)
    res = np.zeros(len(seqs), dtype=np.dtype(capi.CAND_RESULT_DTYPE))
    ex = np.zeros(4096, dtype=np.dtype(capi.FACTOR_DTYPE))
    rp, ep = res.ctypes.data_as(C.POINTER(capi.CandResult)), ex.ctypes.data_as(C.POINTER(capi.Factor))

    def run_c(L, mi=40, p=None):
        prm = capi.CandParams(L, mi)
        return L_.pgpu_pairing_plan_run_candidates(gpu_ctx.h, (p or plan).h, C.byref(prm))

    def fetch(cap=4096, p=None):
        return L_.pgpu_pairing_plan_fetch_candidates(gpu_ctx.h, (p or plan).h, rp, ep, cap)

    def message():
        return L_.pgpu_last_error(gpu_ctx.h).decode()
    try:
        assert fetch() == capi.PGPU_EINVAL and "run_candidates first" in message()          # nothing ran yet
        assert run_c(15) == capi.PGPU_EINVAL and "run_meg" in message()
        plan.run(15, 0.2)
        assert run_c(15) == capi.PGPU_EINVAL and "run_meg" in message()                      # pairings, no records
        plan.run_meg(**M.DEFAULTS)
        assert run_c(0) == capi.PGPU_EINVAL and message() == BAD_PARAMS
        assert run_c((1 << 24) + 1) == capi.PGPU_EINVAL and message() == BAD_PARAMS
        assert run_c(16) == capi.PGPU_EINVAL and "same min_factor_len" in message()          # not the MEG stage's
        assert fetch() == capi.PGPU_EINVAL                                                   # a refused run leaves nothing to fetch
        assert L_.pgpu_pairing_plan_candidate_exons(plan.h) == 0 and plan.candidates_ms() == 0.0
        assert run_c(15) == capi.PGPU_OK
        n = L_.pgpu_pairing_plan_candidate_exons(plan.h)
        assert n > 0 and plan.candidates_ms() > 0.0
        assert fetch(n - 1) == capi.PGPU_ENOSPC and fetch(0) == capi.PGPU_ENOSPC
        assert fetch(n) == capi.PGPU_OK
        want = (res.copy(), ex[:n].copy())
        same(want, CL.expect_arrays([CL.candidate(r, genomic, 15, 40) for r in plan.fetch_meg()]))
        assert L_.pgpu_pairing_plan_run_candidates(gpu_ctx.h, plan.h, None) == capi.PGPU_EINVAL
        assert L_.pgpu_pairing_plan_run_candidates(gpu_ctx.h, None, C.byref(capi.CandParams(15, 40))) == capi.PGPU_EINVAL
        assert L_.pgpu_pairing_plan_fetch_candidates(gpu_ctx.h, plan.h, None, ep, 4096) == capi.PGPU_EINVAL
        assert L_.pgpu_pairing_plan_candidate_exons(None) == 0 and L_.pgpu_pairing_plan_candidates_ms(None) == 0.0
        assert run_c(15) == capi.PGPU_OK and fetch(n) == capi.PGPU_OK
        assert res.tobytes() == want[0].tobytes() and ex[:n].tobytes() == want[1].tobytes()
        plan.run(15, 0.2)                                                                    # a new run: the records are gone
        assert run_c(15) == capi.PGPU_EINVAL and "run_meg" in message()
        assert fetch(n) == capi.PGPU_EINVAL
    finally:
        plan.close()
    # two resident plans: the one whose results the other's run overwrote
    a = capi.PairingPlan(gpu_ctx, idx, seqs[:30], resident=True)
    b = capi.PairingPlan(gpu_ctx, idx, seqs[30:], resident=True)
    try:
        for p in (a, b):
            p.run(15, 0.2)
            p.run_meg(**M.DEFAULTS)
            p.run_candidates(15, 40)
        assert fetch(p=a) == capi.PGPU_EINVAL and "overwritten" in message()          # a's results, then a's records
        assert run_c(15, p=a) == capi.PGPU_EINVAL and "overwritten" in message()
        assert fetch(p=a) == capi.PGPU_EINVAL and "run_candidates first" in message()  # a refused run leaves nothing to fetch
        rb, eb = b.fetch_candidates()
        recs_b = b.fetch_meg()
        same((rb, eb), CL.expect_arrays([CL.candidate(r, genomic, 15, 40) for r in recs_b]))
        a.run(15, 0.2)
        a.run_meg(**M.DEFAULTS)
        a.run_candidates(15, 40)
        ra, ea = a.fetch_candidates()
        same((ra, ea), CL.expect_arrays([CL.candidate(r, genomic, 15, 40) for r in a.fetch_meg()]))
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
            assert gpu_ctx.L.pgpu_pairing_plan_run_candidates(gpu_ctx.h, plan.h, C.byref(prm)) == capi.PGPU_OK
            assert gpu_ctx.L.pgpu_pairing_plan_candidate_exons(plan.h) == 0 and plan.candidates_ms() == 0.0
            assert gpu_ctx.L.pgpu_pairing_plan_fetch_candidates(gpu_ctx.h, plan.h, None, None, 0) == capi.PGPU_OK
        finally:
            plan.close()
    idx.close()


# ---- the index form's contract ------------------------------------------------------------------------------------
def test_refusals_and_the_contract_of_the_index_form(golden, gpu_ctx):
    import pintron_amd.capi as capi
    L_ = gpu_ctx.L
    seqs, groups, idxs = golden
    g, idx = seqs["hand"], idxs["hand"]
    glen = len(g)
    cases = [c for c in groups[("hand", 15, 40)]]
    recs = [c["record"] for c in cases]
    want = CL.expect_arrays(answers(cases))
    n_ex = len(want[1])
    assert n_ex > 10
    blob, first = CL.batch(recs)
    f = L_.pgpu_index_candidates

    def raw(blob_, first_, n, L=15, mi=40, cap=None, blob_len=None):
        """the call with its outputs filled beforehand -> (rc, whether anything was written, *n_exons, outputs)"""
        cap = n_ex if cap is None else cap
        res = np.full(16 * max(n, 1), 0x55, dtype=np.uint8).view(np.dtype(capi.CAND_RESULT_DTYPE))
        ex = np.full(16 * max(cap, 1), 0x55, dtype=np.uint8).view(np.dtype(capi.FACTOR_DTYPE))
        total = C.c_size_t(12345)
        prm = capi.CandParams(L, mi)
        rc = f(gpu_ctx.h, idx.h, blob_, len(blob_) if blob_len is None else blob_len, first_.ctypes.data_as(C.POINTER(C.c_uint64)), n,
               C.byref(prm), res.ctypes.data_as(C.POINTER(capi.CandResult)), ex.ctypes.data_as(C.POINTER(capi.Factor)), cap, C.byref(total))
        untouched = all((x.view(np.uint8) == 0x55).all() for x in (res, ex))
        return rc, untouched, total.value, (res, ex)

    def good():
        rc, _, total, (res, ex) = raw(blob, first, len(recs))
        assert rc == capi.PGPU_OK and total == n_ex
        same((res, ex[:n_ex]), want)
        assert idx.candidates_kernel_ms() > 0.0

    def refused(blob_, first_, n, message=BAD_RECORD, **kw):
        good()                                                                   # a slot for the refusal to reset
        rc, untouched, total, _ = raw(blob_, first_, n, **kw)
        assert rc == capi.PGPU_EINVAL and untouched and total == 12345
        assert CL.einval(blob_[:kw.get("blob_len", len(blob_))], first_, glen, kw.get("L", 15))
        assert L_.pgpu_last_error(gpu_ctx.h).decode() == message and idx.candidates_kernel_ms() == 0.0

    refused(blob, first, len(recs), message=BAD_PARAMS, L=0)
    refused(blob, first, len(recs), message=BAD_PARAMS, L=(1 << 24) + 1)
    refused(blob, first, len(recs), blob_len=len(blob) - 4)                      # the last record runs past the buffer
    for k, value in ((3, int(first[2]) - 4), (len(recs), len(blob) + 4), (5, int(first[5]) + 2)):
        o = first.copy()
        o[k] = value
        refused(blob, o, len(recs))
    # one malformed record in the middle of the batch: each way the header lists
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
        assert CL.record_einval(r, glen), k
        assert len(r) % 4 == 0
        b2, f2 = CL.batch(recs[:7] + [r] + recs[7:])
        refused(b2, f2, len(recs) + 1)
    # a record that is not at a multiple of 4
    shifted = first.copy()
    shifted[1:] += 2
    refused(blob[:int(first[1])] + b"\0\0" + blob[int(first[1]):], shifted, len(recs))
    # PGPU_ENOSPC: the count, and nothing written
    for cap in (0, n_ex - 1):
        good()
        rc, untouched, total, _ = raw(blob, first, len(recs), cap=cap)
        assert rc == capi.PGPU_ENOSPC and untouched and total == n_ex and idx.candidates_kernel_ms() == 0.0
    # null pointers: a bare refusal, the message stays
    good()
    rc, _, _, _ = raw(blob, first, len(recs), L=0)
    res = np.zeros(len(recs), dtype=np.dtype(capi.CAND_RESULT_DTYPE))
    ex = np.zeros(n_ex, dtype=np.dtype(capi.FACTOR_DTYPE))
    total = C.c_size_t(0)
    prm = capi.CandParams(15, 40)
    fp, rp, ep = first.ctypes.data_as(C.POINTER(C.c_uint64)), res.ctypes.data_as(C.POINTER(capi.CandResult)), ex.ctypes.data_as(C.POINTER(capi.Factor))
    full = [gpu_ctx.h, idx.h, blob, len(blob), fp, len(recs), C.byref(prm), rp, ep, n_ex, C.byref(total)]
    for k in (0, 1, 2, 4, 6, 7, 8, 10):
        args = list(full)
        args[k] = None
        assert f(*args) == capi.PGPU_EINVAL, k
        if k:
            assert L_.pgpu_last_error(gpu_ctx.h).decode() == BAD_PARAMS and idx.candidates_kernel_ms() == 0.0
    # n == 0
    good()
    total.value = 99
    assert f(gpu_ctx.h, idx.h, None, 0, None, 0, C.byref(prm), None, None, 0, C.byref(total)) == capi.PGPU_OK
    assert total.value == 0 and idx.candidates_kernel_ms() == 0.0
    # a batch without a candidate: no exon, no buffer needed
    total.value = 99
    none = [CL.bare(CL.UNAVAILABLE), hand_record(cases, "branch")]
    b0, f0 = CL.batch(none)
    assert f(gpu_ctx.h, idx.h, b0, len(b0), f0.ctypes.data_as(C.POINTER(C.c_uint64)), 2, C.byref(prm), rp, None, 0, C.byref(total)) == capi.PGPU_OK
    assert total.value == 0 and list(res["kind"][:2]) == [CL.NONE, CL.NOT_PATH]
    good()                                                                       # the context still answers


def hand_record(cases, name):
    return next(c["record"] for c in cases if c["name"] == name)


def test_without_timing_the_answers_are_the_same(golden):
    import pintron_amd.capi as capi
    seqs, groups, _ = golden
    cases = groups[("hand", 15, 40)]
    recs = [c["record"] for c in cases]
    want = CL.expect_arrays(answers(cases))
    gfa, efa = M.rerun_input()
    exp, genomic = M.first_attempt_megs(gfa, efa)
    with capi.Context(0) as ctx:
        idx = capi.Index(ctx, seqs["hand"])
        same(idx.candidates(recs, 15, 40), want)
        assert idx.candidates_kernel_ms() > 0.0
        ctx.L.pgpu_set_timing(ctx.h, 0)
        same(idx.candidates(recs, 15, 40), want)
        assert idx.candidates_kernel_ms() == 0.0
        idx.close()
        idx = capi.Index(ctx, genomic)
        plan = capi.PairingPlan(ctx, idx, [e["seq"] for e in exp])       # made with timing off: it has no events
        got = run_plan(plan, M.DEFAULTS)
        assert plan.candidates_ms() == 0.0
        same(got, CL.expect_arrays([CL.candidate(r, genomic, 15, 40) for r in plan.fetch_meg()]))
        plan.close()
        idx.close()


# ---- edges by hand ------------------------------------------------------------------------------------------------
def test_edges_by_hand(golden):
    seqs, groups, idxs = golden
    g, idx = seqs["hand"], idxs["hand"]
    cases = groups[("hand", 15, 40)] + groups[("hand", 15, 0)]
    by_name = {c["name"]: c for c in cases}

    def check(names, L=15, mi=40):
        recs = [by_name[n]["record"] if isinstance(n, str) else n for n in names]
        want = CL.expect_arrays([CL.candidate(r, g, L, mi) for r in recs])
        same(idx.candidates(recs, L, mi), want, names[:3])
        return want

    # one record; 64 vertices, numbered along the path and against it
    r, e = check(["split_odd"])
    assert r["kind"][0] == CL.ONE and len(e) == 1
    r, e = check(["vertices_64"])
    assert (r["kind"][0], r["n_pairs"][0], r["work"][0]) == (CL.ONE, 62, 127)
    check(["vertices_64_backwards", "vertices_64_introns", "vertices_64"])
    # the nearest a scan comes to either end of the sequence (min_intron_length 0)
    r, e = check(["node_at_sequence_end", "head_at_sequence_start"], mi=0)
    assert list(r["kind"]) == [CL.ONE, CL.ONE] and e["GEN_end"][0] == len(g) - 1 and e["GEN_start"][1] == 5
    # every third record flagged
    ones = [n for n in ("tie_0", "split_even", "clamp_head", "empty_range_2", "split_odd", "path_out_of_order")]
    names = []
    for k in range(30):
        names.append(CL.bare(CL.UNAVAILABLE if k % 2 else CL.TOO_COMPLEX) if k % 3 == 2 else ones[k % len(ones)])
    r, e = check(names)
    assert list(r["kind"][2::3]) == [CL.NONE] * 10 and not r["n_exons"][2::3].any()
    # 65 records: the last wave has one live thread, and it has work to do
    names = [("tie_%d" % (k % 5)) if k % 2 else "branch" for k in range(64)] + ["vertices_64"]
    r, e = check(names)
    assert r["kind"][64] == CL.ONE and r["first_exon"][64] == len(e) - 1
    # 64 and 63: no partial wave, and one dead lane
    check(names[:64])
    check(names[1:64])
