"""GPU: the list stage -- pgpu_index_factorization_lists against the fixture tests/golden/factorization_lists.json.gz byte
for byte across its four outputs, the hand-made cases in every company, a HOST record between DONE neighbours, the cap
edges inside a batch, the entry's refusals and both PGPU_ENOSPC shapes, with and without timing, the route
pgpu_index_candidate_lists -> this entry against the call-by-call route over the three chained entries with the merge in
Python, the plan form (run -> run_meg -> run_candidate_lists -> run_factorization_lists) against the restatement
(tests/flists_lib.py) on the device's own lists, against the index form and against the factorization stage, and the rules
of the branch.  Every comparison is byte equality."""
import ctypes as C

import numpy as np
import pytest

import cand_lib as CL
import enum_lib as EL
import fact_lib as FL
import flists_lib as F
import meg_lib as M

pytestmark = pytest.mark.gpu

NAMES = ("results", "facts", "exons", "steps")


def same(got, want, what=""):
    for name, g, w in zip(NAMES, got, want):
        assert len(g) == len(w), (what, name, len(g), len(w))
        if g.tobytes() != w.tobytes():
            bad = [i for i in range(len(g)) if g[i] != w[i]]
            raise AssertionError("%s: %s differ at %d places, first %d: %r / %r" % (what, name, len(bad), bad[0], g[bad[0]], w[bad[0]]))


@pytest.fixture(scope="module")
def golden(gpu_ctx):
    """the fixture, grouped: {(sequence, settings): [case]}, and one index per sequence"""
    import pintron_amd.capi as capi
    seqs, cases, _ = F.load_fixture()
    groups = {}
    for c in cases:
        groups.setdefault((c["seq"], c["prm"]), []).append(c)
    idx = {name: capi.Index(gpu_ctx, seqs[name]) for name in {c["seq"] for c in cases}}
    yield seqs, groups, idx
    for i in idx.values():
        i.close()


def call(idx, cases, prm):
    """one call over the cases: (got, want)"""
    ests, cands, exons, q = F.batch_arrays([(c["est"], c["cands"]) for c in cases])
    got = idx.factorization_lists(ests, cands, exons, q, F.capi_params(prm))
    return got, F.expect_arrays([c["answer"] for c in cases], q["first_candidate"])


def test_every_golden_case_one_call_per_parameter_set_and_again(golden):
    seqs, groups, idx = golden
    assert sum(len(g) for g in groups.values()) > 800
    for (seq, prm), cases in groups.items():
        got, want = call(idx[seq], cases, prm)
        same(got, want, (seq, prm))
        assert idx[seq].factorization_lists_kernel_ms() > 0.0     # the fixture's context has timing on
        again, _ = call(idx[seq], cases, prm)
        assert F.same_arrays(again, got), (seq, prm)


def test_golden_cases_on_a_loaded_index(golden, gpu_ctx, tmp_path):
    import pintron_amd.capi as capi
    seqs, groups, idx = golden
    for seq in ("hand", "issue13"):
        path = str(tmp_path / (seq + ".idx"))
        idx[seq].save(path)
        loaded = capi.Index(gpu_ctx, seqs[seq], load_from=path)
        try:
            for (s, prm), cases in groups.items():
                if s == seq:
                    same(*call(loaded, cases, prm), what=(seq, prm))
        finally:
            loaded.close()


def hand(golden, prm=F.DEFAULTS):
    seqs, groups, idxs = golden
    return idxs["hand"], [c for c in groups[("hand", prm)]]


def test_hand_made_cases_in_one_batch_reversed_and_one_by_one(golden):
    seqs, groups, idxs = golden
    n = 0
    for (seq, prm), cases in groups.items():
        if seq not in ("hand", "fact"):
            continue
        same(*call(idxs[seq], cases[::-1], prm), what=("reversed", prm))
        for c in cases:                                            # an answer never depends on its neighbours
            same(*call(idxs[seq], [c], prm), what=c["name"])
        n += len(cases)
    assert n > 90


def test_a_host_record_between_done_neighbours_and_the_cap_edges_inside_a_batch(golden):
    idx, cases = hand(golden)
    by_name = {c["name"]: c for c in cases}
    done = [by_name["hand/" + n] for n in ("different", "widen_both", "contained", "one_equal")]
    hosts = [by_name["hand/" + n] for n in ("refused_second", "cap_first_of_two_bad", "gaps_cap_alone", "cands_65", "cands_64")]
    batch = []
    for k, h in enumerate(hosts):
        batch += [done[k % len(done)], h]
    batch.append(done[0])
    got, want = call(idx, batch, F.DEFAULTS)
    same(got, want)
    res = got[0]
    assert [(int(r["outcome"]), int(r["stage"]), int(r["detail"])) for r in res[1::2]] == \
        [(F.HOST, 1, 2), (F.HOST, 1, 1), (F.HOST, 3, 1), (F.HOST, 0, F.CAP_CANDIDATES), (F.DONE, 4, 0)]
    assert all(int(r["outcome"]) == F.DONE for r in res[::2])
    assert int(res[9]["n_facts"]) == 64 and int(res[9]["n_listed"]) == 64


def test_kept_exons_out_of_order_are_host_at_stage_4_over_gaps_results_made_by_hand(golden, gpu_ctx):
    """gaps_kernel cannot write two kept exons that are not strictly in order (flists_lib, beside TAGS), so the order test of
    flist_gaps_to_refine_kernel and the HOST branch of the gather are run through pgpu_flist_handoffs_probe: the entry with
    gaps' three outputs given.  Given what gaps computes on exact exons (the exons unchanged, no step, no error) the answer
    is the entry's own; with one exon moved it is what the restatement says over the same given results."""
    import pintron_amd.capi as capi
    idx, cases = hand(golden)
    by_name = {c["name"]: c for c in cases}
    batch = [by_name["hand/" + n] for n in ("one_candidate", "different", "contained", "different", "one_equal")]
    ests, cands, exons, q = F.batch_arrays([(c["est"], c["cands"]) for c in batch])
    E, n_c = len(exons), len(cands)
    prm = F.capi_params(F.DEFAULTS)

    def given(change=None, merged=()):
        gr, gx, gs = given_arrays_of(capi, cands, exons)
        for at, field, value in (change or ()):
            gx[field][at] = value
        for at in merged:
            gs[at] = 0x80
        dicts = []
        for i in range(len(batch)):
            d = {}
            for j in range(int(q["n_candidates"][i])):
                c = int(q["first_candidate"][i]) + j
                a, n = int(cands["first_exon"][c]), int(cands["n_exons"][c])
                d[j] = (0, 0, 0, [tuple(int(v) for v in e) for e in gx[a:a + n].tolist()], [int(s) for s in gs[a:a + n]])
            dicts.append(d)
        want = F.expect_arrays([F.factorization_list(c["est"], golden[0]["hand"], c["cands"], F.DEFAULTS, given_gaps=d)
                                for c, d in zip(batch, dicts)], q["first_candidate"])
        rc, *got = capi.flist_handoffs_probe(gpu_ctx, idx, ests, cands, exons, q, prm, gr, gx, gs)
        assert rc == capi.PGPU_OK
        return tuple(got), want

    # what gaps computes here, given: the entry's own answer
    got, want = given()
    same(got, want, "unchanged")
    same(got, idx.factorization_lists(ests, cands, exons, q, prm), "the entry itself")
    assert all(int(r["outcome"]) == F.DONE for r in got[0])
    # EST 1 (`different`: [a, b] and [c, d]): d begins where c begins on the sequence -- the second entry is out of order
    c1 = int(q["first_candidate"][1]) + 1
    at = int(cands["first_exon"][c1])
    got, want = given([(at + 1, "GEN_start", int(exons["GEN_start"][at]))])
    same(got, want, "second entry out of order")
    assert [(int(r["outcome"]), int(r["stage"]), int(r["detail"])) for r in got[0]] == \
        [(F.DONE, 4, 0), (F.HOST, 4, 2), (F.DONE, 4, 0), (F.DONE, 4, 0), (F.DONE, 4, 0)]
    assert tuple(int(got[0][1][k]) for k in ("n_cleaned", "n_listed", "n_filtered", "n_facts")) == (2, 2, 2, 0)
    # ... on the EST alone: equal ends (EST_end == EST_start) are out of order too; the first entry decides as well as the second
    c0 = int(q["first_candidate"][3])
    a0 = int(cands["first_exon"][c0])
    got, want = given([(a0 + 1, "EST_start", int(exons["EST_end"][a0]))])
    same(got, want, "first entry out of order on the EST")
    assert (int(got[0][3]["outcome"]), int(got[0][3]["stage"]), int(got[0][3]["detail"])) == (F.HOST, 4, 2)
    assert int(got[0][1]["outcome"]) == F.DONE
    # an exon gaps marked merged is not among the kept ones: the same move under bit 7 is no violation
    got, want = given([(at + 1, "GEN_start", int(exons["GEN_start"][at]))], merged=[at + 1])
    same(got, want, "the moved exon merged")
    assert int(got[0][1]["outcome"]) == F.DONE and int(got[1][int(got[0][1]["first_fact"]) + 1]["n_merged"]) == 1
    # null pointers
    f = gpu_ctx.L.pgpu_flist_handoffs_probe
    assert capi.flist_handoffs_probe(gpu_ctx, idx, ests, cands, exons, q, prm, *given_arrays_of(capi, cands, exons))[0] == capi.PGPU_OK
    assert f(gpu_ctx.h, idx.h, ests, len(ests), None, 0, None, 0, None, 0, C.byref(prm), None, None, 0, None, None, 0, None, None,
             None, None, None) == capi.PGPU_EINVAL


def given_arrays_of(capi, cands, exons):
    """gaps' three outputs when it has nothing to do: every exon unchanged, a placeholder per candidate, no step, no error"""
    gr = np.zeros(len(cands), dtype=np.dtype(capi.GAPS_RESULT_DTYPE))
    gr["n_kept"] = cands["n_exons"]
    ph = np.full(4 * len(cands), -1, dtype="<i4").view(np.dtype(capi.FACTOR_DTYPE))
    return gr, np.concatenate([exons, ph]), np.zeros(len(exons) + len(cands), dtype=np.uint8)


def test_refusals_and_both_enospc_shapes(golden, gpu_ctx):
    import pintron_amd.capi as capi
    idx, cases = hand(golden)
    cases = cases[:24]
    ests, cands, exons, q = F.batch_arrays([(c["est"], c["cands"]) for c in cases])
    want = F.expect_arrays([c["answer"] for c in cases], q["first_candidate"])
    n_f, n_e = len(want[1]), len(want[2])
    assert n_f > 10 and n_e > n_f

    def raw(ests_=ests, cands_=cands, exons_=exons, q_=q, prm=None, fcap=n_f, ecap=n_e):
        return idx.factorization_lists_raw(ests_, cands_, exons_, q_, len(q_), prm or F.capi_params(F.DEFAULTS), fcap, ecap)

    def refused(**kw):
        rc = raw(**kw)[0]
        return rc == capi.PGPU_EINVAL and idx.factorization_lists_kernel_ms() == 0.0

    rc, res, facts, ex, st, nf, ne = raw()
    assert rc == capi.PGPU_OK and (nf, ne) == (n_f, n_e)
    same((res, facts[:nf], ex[:ne], st[:ne]), want)
    # both PGPU_ENOSPC shapes: the needed counts come back, nothing is written
    for fcap, ecap in ((n_f - 1, n_e), (n_f, n_e - 1), (0, 0)):
        rc, res, facts, ex, st, nf, ne = raw(fcap=fcap, ecap=ecap)
        assert rc == capi.PGPU_ENOSPC and (nf, ne) == (n_f, n_e)
        assert not res.view(np.uint8).any() and not facts.view(np.uint8).any() and not ex.view(np.uint8).any() and not st.any()

    def changed(arr, i, field, value):
        out = arr.copy()
        out[field][i] = value
        return out
    assert refused(q_=changed(q, 3, "reserved", 1))
    assert refused(q_=changed(q, 3, "est_len", 0))
    assert refused(q_=changed(q, 3, "est_off", len(ests)))
    assert refused(q_=changed(q, 3, "n_candidates", len(cands) + 1))
    assert refused(q_=changed(q, 3, "first_candidate", int(q["first_candidate"][2])))          # two queries share a candidate
    assert refused(cands_=changed(cands, 5, "reserved", 1))
    assert refused(cands_=changed(cands, 5, "n_exons", 0))
    assert refused(cands_=changed(cands, 5, "first_exon", len(exons)))
    assert refused(cands_=changed(cands, 5, "first_exon", int(cands["first_exon"][4])))         # two candidates share an exon
    for kw in (dict(max_coverage_diff=1.5), dict(max_coverage_diff=-0.1), dict(max_coverage_diff=float("nan")),
               dict(max_site_difference=-1), dict(max_site_difference=(1 << 24) + 1), dict(max_gaplength_diff=-2),
               dict(max_number_of_factorizations=-1), dict(suffpref_length_on_est=-1), dict(reserved=1)):
        assert refused(prm=capi.flist_params(**kw)), kw
    # a candidate no query names is not looked at
    rc, res, facts, ex, st, nf, ne = raw(cands_=np.concatenate([cands, changed(cands[:1], 0, "n_exons", 0)]))
    assert rc == capi.PGPU_OK
    same((res, facts[:nf], ex[:ne], st[:ne]), want)
    # null pointers: a bare PGPU_EINVAL
    f = gpu_ctx.L.pgpu_index_factorization_lists
    prm = F.capi_params(F.DEFAULTS)
    nfc, nec = C.c_size_t(0), C.c_size_t(0)
    args = [gpu_ctx.h, idx.h, ests, len(ests), cands.ctypes.data_as(C.POINTER(capi.EnumCandidate)), len(cands),
            exons.ctypes.data_as(C.POINTER(capi.Factor)), len(exons), q.ctypes.data_as(C.POINTER(capi.FlistQuery)), len(q), C.byref(prm),
            res.ctypes.data_as(C.POINTER(capi.FlistResult)), facts.ctypes.data_as(C.POINTER(capi.FlistFact)), n_f,
            ex.ctypes.data_as(C.POINTER(capi.Factor)), st.ctypes.data_as(C.POINTER(C.c_uint8)), n_e, C.byref(nfc), C.byref(nec)]
    for k in (0, 1, 2, 4, 6, 8, 10, 11, 12, 14, 15, 17, 18):
        bad = list(args)
        bad[k] = None
        assert f(*bad) == capi.PGPU_EINVAL, k
    # the empty call
    empty_q = q[:0]
    rc, res0, _, _, _, nf, ne = idx.factorization_lists_raw(b"", cands[:0], exons[:0], empty_q, 0, prm, 0, 0)
    assert rc == capi.PGPU_OK and (nf, ne) == (0, 0)
    rc, res, facts, ex, st, nf, ne = raw()                                          # the context still answers
    assert rc == capi.PGPU_OK
    same((res, facts[:nf], ex[:ne], st[:ne]), want)


def test_without_timing_the_answers_are_the_same(golden):
    import pintron_amd.capi as capi
    seqs, groups, _ = golden
    cases = groups[("hand", F.DEFAULTS)]
    with capi.Context(0) as ctx:
        idx = capi.Index(ctx, seqs["hand"])
        same(*call(idx, cases, F.DEFAULTS))
        assert idx.factorization_lists_kernel_ms() > 0.0
        ctx.L.pgpu_set_timing(ctx.h, 0)
        same(*call(idx, cases, F.DEFAULTS))
        assert idx.factorization_lists_kernel_ms() == 0.0
        idx.close()


# ---- candidate lists -> this entry, against the call-by-call route --------------------------------------------------------
def call_by_call(idx, gen_len, ests, cands, exons, q, prm):
    """the same arrays from pgpu_index_clean_chains, the merge and the filters in Python (flists_lib), pgpu_index_gap_chains
    and pgpu_index_refine_chains, one call each over every EST's candidates"""
    from pintron_amd import capi
    thr, settings = prm[0], tuple(prm[1:5])
    answers = [None] * len(q)
    # clean: one query per candidate of every EST that has 1 .. 64 candidates with good input
    live, cq_rows = [], []
    for i in range(len(q)):
        m, fc = int(q["n_candidates"][i]), int(q["first_candidate"][i])
        if m == 0:
            answers[i] = F.answer(F.EMPTY, 0, 0)
        elif m > F.MAX_CANDIDATES:
            answers[i] = F.answer(F.HOST, 0, F.CAP_CANDIDATES)
        else:
            bad = False
            for c in range(fc, fc + m):
                ex = [tuple(int(v) for v in e) for e in exons[int(cands["first_exon"][c]):int(cands["first_exon"][c]) + int(cands["n_exons"][c])].tolist()]
                one = [dict(est_off=0, est_len=int(q["est_len"][i]), first_exon=0, n_exons=len(ex), reserved=0)]
                if F.CL.einval(int(q["est_len"][i]), gen_len, ex, one):
                    bad = True
            if bad:                                                # the lowest index decides: a cap in front of the refused input?
                answers[i] = F.answer(F.HOST, 1, 1 if any_cap_first(idx, ests, cands, exons, q, i, thr, gen_len) else 2)
            else:
                live.append(i)
                cq_rows += [(int(q["est_off"][i]), int(q["est_len"][i]), int(cands["first_exon"][c]), int(cands["n_exons"][c]), 0, thr)
                            for c in range(fc, fc + m)]
    cq = np.array(cq_rows, dtype=np.dtype(capi.CLEAN_QUERY_DTYPE)).reshape(-1)
    ex2, _, cres = idx.clean_chains(ests, exons, cq) if len(cq) else (exons, None, cq)
    # the merge and the filters on the host, then gaps and refine per entry
    k = 0
    stage = {}
    for i in live:
        m, fc = int(q["n_candidates"][i]), int(q["first_candidate"][i])
        rows = list(range(k, k + m))
        k += m
        if any(int(cres["status"][r]) != 0 for r in rows):
            answers[i] = F.answer(F.HOST, 1, 1)
            continue
        survivors = []
        for j, r in enumerate(rows):
            if int(cres["verdict"][r]) == 0:
                at = int(cq["first_exon"][r]) + int(cres["first_kept"][r])
                survivors.append(dict(idx=j, exons=[list(int(v) for v in e) for e in ex2[at:at + int(cres["n_kept"][r])].tolist()], flags=0))
        if not survivors:
            answers[i] = F.answer(F.EMPTY, 1, 0)
            continue
        flist = []
        for e in survivors:
            F.add_if_not_exists(flist, e, int(prm[6]), {})
        n_listed = len(flist)
        flist = F.filter3(F.filter1(flist, int(q["est_len"][i]), prm[5], {}), prm[7], {})
        stage[i] = (flist, (len(survivors), n_listed, len(flist)))
    # gaps
    gex, gq_rows, owner = [], [], []
    for i, (flist, counts) in stage.items():
        for e in flist:
            lst = [tuple(x) for x in e["exons"]]
            one = [dict(est_off=0, est_len=int(q["est_len"][i]), first_exon=0, n_exons=len(lst), reserved=0)]
            if F.GL.einval(int(q["est_len"][i]), gen_len, lst, one):
                answers[i] = answers[i] or F.answer(F.HOST, 3, 2, counts)
                e["bad"] = True
                continue
            gq_rows.append((int(q["est_off"][i]), int(q["est_len"][i]), len(gex), len(lst), 0))
            owner.append((i, e))
            gex += lst
    gq = np.array(gq_rows, dtype=np.dtype(capi.GAPS_QUERY_DTYPE)).reshape(-1)
    gexa = np.array(gex, dtype=np.dtype(capi.FACTOR_DTYPE)).reshape(-1)
    if len(gq):
        ex3, gsteps, gres = idx.gap_chains(ests, gexa, gq)
    rex, rq_rows, rowner = [], [], []
    for r, (i, e) in enumerate(owner):
        e["gaps"] = r
    for i, (flist, counts) in stage.items():
        left = []
        for e in flist:                                            # the lowest index decides
            if e.get("bad"):
                answers[i] = F.answer(F.HOST, 3, 2, counts)
                break
            r = e["gaps"]
            if int(gres["status"][r]) != 0:
                answers[i] = F.answer(F.HOST, 3, 1, counts)
                break
            if int(gres["verdict"][r]) != 0:
                continue
            at, n = int(gq["first_exon"][r]), int(gq["n_exons"][r])
            kept = [tuple(int(v) for v in x) for x, s in zip(ex3[at:at + n].tolist(), gsteps[at:at + n]) if not s & F.MERGED]
            left.append(dict(e, exons=kept, n_merged=n - len(kept), total_edit=int(gres["total_edit"][r])))
        else:
            if not left:
                answers[i] = F.answer(F.EMPTY, 3, 1, counts)
            elif prm[8] != 0 and len(left) > prm[8]:
                answers[i] = F.answer(F.EMPTY, 3, 2, counts)
            else:
                stage[i] = (left, counts)
                continue
        stage[i] = None
    for i, v in stage.items():
        if v is None:
            continue
        left, counts = v
        for e in left:
            lst = e["exons"]
            if any(d[1] >= a[0] or d[3] >= a[2] for d, a in zip(lst, lst[1:])):
                e["bad"] = True
                continue
            e["refine"] = len(rq_rows)
            rq_rows.append((int(q["est_off"][i]), int(q["est_len"][i]), len(rex), len(lst), 0) + settings)
            rex += lst
    rq = np.array(rq_rows, dtype=np.dtype(capi.CHAIN_QUERY_DTYPE)).reshape(-1)
    rexa = np.array(rex, dtype=np.dtype(capi.FACTOR_DTYPE)).reshape(-1)
    if len(rq):
        ex4, rsteps, rres = idx.refine_chains(ests, rexa, rq)
    for i, v in stage.items():
        if v is None:
            continue
        left, counts = v
        facts = []
        for e in left:
            if e.get("bad"):
                answers[i] = F.answer(F.HOST, 4, 2, counts)
                break
            r = e["refine"]
            if int(rres["status"][r]) != 0:
                answers[i] = F.answer(F.HOST, 4, 1, counts)
                break
            at, n, dropped = int(rq["first_exon"][r]), int(rq["n_exons"][r]), int(rres["dropped_first"][r])
            facts.append(dict(candidate=e["idx"], exons=[tuple(int(v) for v in x) for x in ex4[at + dropped:at + n].tolist()],
                              steps=[int(s) for s in rsteps[at + dropped:at + n]], n_merged=e["n_merged"], total_edit=e["total_edit"],
                              flags=e["flags"] | (F.DROPPED_FIRST if dropped else 0)))
        else:
            answers[i] = F.answer(F.DONE, 4, 0, counts, facts)
    return F.expect_arrays(answers, q["first_candidate"])


def any_cap_first(idx, ests, cands, exons, q, i, thr, gen_len):
    """whether, among EST i's candidates, one that clean refuses for a cap comes in front of the first refused input (the
    lowest index decides): the candidates in front of that input, through pgpu_index_clean_chains"""
    from pintron_amd import capi
    fc, m = int(q["first_candidate"][i]), int(q["n_candidates"][i])
    rows = []
    for c in range(fc, fc + m):
        ex = [tuple(int(v) for v in e) for e in exons[int(cands["first_exon"][c]):int(cands["first_exon"][c]) + int(cands["n_exons"][c])].tolist()]
        one = [dict(est_off=0, est_len=int(q["est_len"][i]), first_exon=0, n_exons=len(ex), reserved=0)]
        if F.CL.einval(int(q["est_len"][i]), gen_len, ex, one):
            break
        rows.append((int(q["est_off"][i]), int(q["est_len"][i]), int(cands["first_exon"][c]), int(cands["n_exons"][c]), 0, thr))
    if not rows:
        return False
    cq = np.array(rows, dtype=np.dtype(capi.CLEAN_QUERY_DTYPE)).reshape(-1)
    return bool((idx.clean_chains(ests, exons, cq)[2]["status"] != 0).any())


def test_candidate_lists_into_this_entry_against_the_call_by_call_route(golden, gpu_ctx):
    import pintron_amd.capi as capi
    seqs, groups, idxs = golden
    # the enumeration stage's output as it is: the real records of one parameter set, their ESTs beside them
    _, ecases, _ = EL.load_fixture()
    picked = [c for c in ecases if c["seq"] == "issue13" and c["name"].split("/")[1] == "defaults"]
    assert len(picked) > 150
    idx = idxs["issue13"]
    res, cands, exons = idx.candidate_lists([c["record"] for c in picked], 15, 40)
    ests_of = F.real_ests()[("issue13", "defaults")]
    ests, off = [], [0]
    for c in picked:
        ests.append(ests_of[int(c["name"].split("/")[2])])
        off.append(off[-1] + len(ests[-1]))
    q = np.zeros(len(picked), dtype=np.dtype(capi.FLIST_QUERY_DTYPE))
    q["est_off"], q["est_len"] = off[:-1], np.diff(off)
    lists = res["kind"] == EL.LISTS
    q["first_candidate"] = np.where(lists, res["first_candidate"], 0)
    q["n_candidates"] = np.where(lists, res["n_candidates"], 0)
    blob = b"".join(ests)
    got = idx.factorization_lists(blob, cands, exons, q, F.capi_params(F.DEFAULTS))
    same(got, call_by_call(idx, len(seqs["issue13"]), blob, cands, exons, q, F.DEFAULTS), "call by call")
    assert (got[0]["outcome"] == F.DONE).sum() > 100 and (got[0]["n_facts"] >= 2).sum() >= 3
    # and the hand-made cases, whose HOST outcomes the real records do not reach
    hidx, cases = hand(golden)
    e2, c2, x2, q2 = F.batch_arrays([(c["est"], c["cands"]) for c in cases])
    same(hidx.factorization_lists(e2, c2, x2, q2, F.capi_params(F.DEFAULTS)),
         call_by_call(hidx, len(seqs["hand"]), e2, c2, x2, q2, F.DEFAULTS), "call by call, hand-made")


# ---- the plan form ------------------------------------------------------------------------------------------------------
def run_plan(plan, prm, fprm=F.DEFAULTS):
    plan.run(prm["min_factor_len"], 0.2)
    plan.run_meg(**prm)
    plan.run_candidate_lists(prm["min_factor_len"], prm["min_intron_length"])
    plan.run_factorization_lists(F.capi_params(fprm))
    return plan.fetch_factorization_lists()


def restated_plan(genomic, seqs, lists, fprm):
    """the restatement on the device's own fetched candidate lists: the four arrays"""
    res, cands, exons = lists
    answers = []
    for k, est in enumerate(seqs):
        r = res[k]
        if int(r["kind"]) != EL.LISTS:
            answers.append(F.answer(F.HOST, 0, int(r["kind"])))
            continue
        cl = []
        for c in cands[int(r["first_candidate"]):int(r["first_candidate"]) + int(r["n_candidates"])]:
            cl.append([tuple(int(v) for v in e) for e in exons[int(c["first_exon"]):int(c["first_exon"]) + int(c["n_exons"])].tolist()])
        answers.append(F.factorization_list(est, genomic, cl, fprm))
    return F.expect_arrays(answers, np.where(res["kind"] == EL.LISTS, res["first_candidate"], 0)), answers


@pytest.mark.parametrize("source,n_pat", [("c2", 307), ("issue13", 1891)])
@pytest.mark.parametrize("resident", [False, True])
def test_plan_form_against_the_restatement_the_index_form_and_the_factorization_stage(gpu_ctx, source, n_pat, resident):
    import pintron_amd.capi as capi
    gfa, efa = CL.real_inputs()[source]
    prm = M.DEFAULTS
    exp, genomic = M.first_attempt_megs(gfa, efa, prm)
    assert len(exp) == n_pat
    seqs = [e["seq"] for e in exp]
    idx = capi.Index(gpu_ctx, genomic)
    plan = capi.PairingPlan(gpu_ctx, idx, seqs, resident=resident)
    try:
        got = run_plan(plan, prm)
        assert plan.factorization_lists_ms(0) > 0.0 and plan.factorization_lists_ms(2) > 0.0
        assert plan.factorization_list_counts() == (len(got[1]), len(got[2]))
        lists = plan.fetch_candidate_lists()
        want, answers = restated_plan(genomic, seqs, lists, F.DEFAULTS)
        same(got, want, source)
        assert (got[0]["outcome"] == F.DONE).sum() > n_pat // 3
        assert int(lists[0]["n_candidates"].max()) >= 2          # (c2's lists of two are the empty graph's source and sink)
        assert source != "issue13" or (int(got[0]["n_cleaned"].max()) >= 2 and int(got[0]["n_facts"].max()) >= 2)
        # the index form on the fetched lists: byte for byte
        off = np.zeros(n_pat + 1, dtype=np.uint64)
        np.cumsum([len(s) for s in seqs], out=off[1:])
        q = np.zeros(n_pat, dtype=np.dtype(capi.FLIST_QUERY_DTYPE))
        q["est_off"], q["est_len"] = off[:-1], np.diff(off)
        is_lists = lists[0]["kind"] == EL.LISTS
        q["first_candidate"] = np.where(is_lists, lists[0]["first_candidate"], 0)
        q["n_candidates"] = np.where(is_lists, lists[0]["n_candidates"], 0)
        ires = idx.factorization_lists(b"".join(seqs), lists[1], lists[2], q, F.capi_params(F.DEFAULTS))
        # (the index form knows no enumeration kind: a record without lists is EMPTY at stage 0 there)
        fixed = ires[0].copy()
        for k in np.nonzero(~is_lists)[0]:
            fixed[k] = (F.HOST, 0, int(lists[0]["kind"][k]), 0, 0, 0, 0, 0)
        same((fixed,) + tuple(ires[1:]), got, source + " index form")
        # the factorization stage, on every record run_candidates calls ONE: the same outcome and exons
        plan.run_candidates(prm["min_factor_len"], prm["min_intron_length"])
        plan.run_factorizations()
        cres, _ = plan.fetch_candidates()
        fres, fex, fst = plan.fetch_factorizations()
        n_one = 0
        for k in np.nonzero(cres["kind"] == CL.ONE)[0]:
            r, fr = got[0][k], fres[k]
            assert int(r["outcome"]) == int(fr["outcome"]), (source, k)
            if int(fr["outcome"]) == F.DONE:
                assert int(r["n_facts"]) == 1
                ff = got[1][int(r["first_fact"])]
                a, n = int(ff["first_exon"]), int(ff["n_exons"])
                b = int(fr["first_exon"])
                assert n == int(fr["n_exons"]) and got[2][a:a + n].tobytes() == fex[b:b + n].tobytes(), (source, k)
                assert got[3][a:a + n].tobytes() == fst[b:b + n].tobytes(), (source, k)
                n_one += 1
        assert n_one > n_pat // 4
        # the rungs left the branch fetchable and unchanged; a rerun gives the same bytes
        assert F.same_arrays(plan.fetch_factorization_lists(), got)
        assert F.same_arrays(run_plan(plan, prm), got)
    finally:
        plan.close()
        idx.close()


def test_the_branch_rules_and_the_refusals_of_the_plan_form(gpu_ctx):
    import pintron_amd.capi as capi
    L_ = gpu_ctx.L
    gfa, efa = M.rerun_input()
    exp, genomic = M.first_attempt_megs(gfa, efa)
    seqs = [e["seq"] for e in exp]
    idx = capi.Index(gpu_ctx, genomic)
    plan = capi.PairingPlan(gpu_ctx, idx, seqs)

    def run_f(p=None, **kw):
        prm = capi.flist_params(**kw)
        return L_.pgpu_pairing_plan_run_factorization_lists(gpu_ctx.h, (p or plan).h, C.byref(prm))

    def fetch(p=None, fcap=None, ecap=None):
        return (p or plan).fetch_factorization_lists_raw(fcap, ecap)[0]

    def message():
        return L_.pgpu_last_error(gpu_ctx.h).decode()

    def blob(arrays):
        return [np.asarray(a).tobytes() for a in arrays]
    try:
        assert fetch(fcap=0, ecap=0) == capi.PGPU_EINVAL and "run_factorization_lists" in message()      # fetch before run
        assert run_f() == capi.PGPU_EINVAL and "run_candidate_lists" in message()
        plan.run(15, 0.2)
        plan.run_meg(**M.DEFAULTS)
        assert run_f() == capi.PGPU_EINVAL and "run_candidate_lists" in message()                  # records, no lists
        plan.run_candidate_lists(15, 40)
        assert run_f(max_number_of_factorizations=-1) == capi.PGPU_EINVAL and "parameters" in message()
        assert run_f(reserved=1) == capi.PGPU_EINVAL and fetch(fcap=0, ecap=0) == capi.PGPU_EINVAL
        assert plan.factorization_list_counts() == (0, 0) and plan.factorization_lists_ms(0) == 0.0
        # the ladder is climbed first; the branch leaves every rung, and the candidate lists, fetchable and unchanged
        plan.run_candidates(15, 40)
        plan.run_factorizations()
        plan.run_final_factorizations()
        before = blob(plan.fetch_candidates()) + blob(plan.fetch_factorizations()) + blob(plan.fetch_final_factorizations()) + \
            blob(plan.fetch_candidate_lists()) + blob([b"".join(plan.fetch_meg())])
        assert run_f() == capi.PGPU_OK
        n_f, n_e = plan.factorization_list_counts()
        assert n_f > 0 and n_e >= n_f
        after = blob(plan.fetch_candidates()) + blob(plan.fetch_factorizations()) + blob(plan.fetch_final_factorizations()) + \
            blob(plan.fetch_candidate_lists()) + blob([b"".join(plan.fetch_meg())])
        assert before == after
        assert fetch(fcap=n_f - 1, ecap=n_e) == capi.PGPU_ENOSPC and fetch(fcap=n_f, ecap=n_e - 1) == capi.PGPU_ENOSPC
        want = plan.fetch_factorization_lists()
        same(want, restated_plan(genomic, seqs, plan.fetch_candidate_lists(), F.DEFAULTS)[0])
        # the rungs neither need the branch nor disturb it
        plan.run_candidates(15, 40)
        plan.run_factorizations()
        assert F.same_arrays(plan.fetch_factorization_lists(), want)
        # null pointers touch nothing; a refused run takes its results along
        assert L_.pgpu_pairing_plan_run_factorization_lists(gpu_ctx.h, plan.h, None) == capi.PGPU_EINVAL
        assert L_.pgpu_pairing_plan_run_factorization_lists(gpu_ctx.h, None, C.byref(capi.flist_params())) == capi.PGPU_EINVAL
        assert L_.pgpu_pairing_plan_factorization_list_counts(None, None, None) == capi.PGPU_EINVAL
        assert L_.pgpu_pairing_plan_factorization_lists_ms(None, 0) == 0.0
        assert F.same_arrays(plan.fetch_factorization_lists(), want)
        assert run_f(max_gaplength_diff=-2) == capi.PGPU_EINVAL and fetch() == capi.PGPU_EINVAL
        assert run_f() == capi.PGPU_OK and F.same_arrays(plan.fetch_factorization_lists(), want)
        # run_candidate_lists, run_meg and run end them
        plan.run_candidate_lists(15, 40)
        assert fetch() == capi.PGPU_EINVAL and "run_factorization_lists" in message()
        assert run_f() == capi.PGPU_OK and F.same_arrays(plan.fetch_factorization_lists(), want)
        plan.run_meg(**M.DEFAULTS)
        assert fetch() == capi.PGPU_EINVAL and run_f() == capi.PGPU_EINVAL and "run_candidate_lists" in message()
        plan.run_candidate_lists(15, 40)
        assert run_f() == capi.PGPU_OK and F.same_arrays(plan.fetch_factorization_lists(), want)
        plan.run(15, 0.2)
        assert fetch() == capi.PGPU_EINVAL and run_f() == capi.PGPU_EINVAL
    finally:
        plan.close()
    # two resident plans: the one whose results the other's run overwrote
    a = capi.PairingPlan(gpu_ctx, idx, seqs[:30], resident=True)
    b = capi.PairingPlan(gpu_ctx, idx, seqs[30:], resident=True)
    try:
        for p in (a, b):
            run_plan(p, M.DEFAULTS)
        assert fetch(p=a) == capi.PGPU_EINVAL and "overwritten" in message()
        assert run_f(p=a) == capi.PGPU_EINVAL and "overwritten" in message()
        same(b.fetch_factorization_lists(), restated_plan(genomic, seqs[30:], b.fetch_candidate_lists(), F.DEFAULTS)[0])
        got_a = run_plan(a, M.DEFAULTS)
        same(got_a, restated_plan(genomic, seqs[:30], a.fetch_candidate_lists(), F.DEFAULTS)[0])
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
            prm = capi.flist_params()
            assert gpu_ctx.L.pgpu_pairing_plan_run_factorization_lists(gpu_ctx.h, plan.h, C.byref(prm)) == capi.PGPU_OK
            assert plan.factorization_list_counts() == (0, 0) and plan.factorization_lists_ms(0) == 0.0
            assert gpu_ctx.L.pgpu_pairing_plan_fetch_factorization_lists(gpu_ctx.h, plan.h, None, None, 0, None, None, 0) == capi.PGPU_OK
        finally:
            plan.close()
    idx.close()
