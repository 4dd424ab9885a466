"""GPU: the factorization stage -- pgpu_index_factorizations and pgpu_pairing_plan_run_factorizations against the
restatement (tests/fact_lib.py) and against the call-by-call route (the three existing chained entries called one after the
other with the glue on the host).  Every comparison is byte equality: results, exons, step bytes."""
import ctypes as C

import numpy as np
import pytest

import cand_lib as KL
import fact_lib as F
import meg_lib as M

pytestmark = pytest.mark.gpu

BAD_PARAMS = "bad factorization parameters (a suffpref length outside [0, 2^24])"
BAD_QUERY = "bad factorization query (a range past its buffer, an empty EST, reserved != 0, or an exon two queries share)"
FIXTURES = ("clean_chains", "gap_chains", "refine_chains")


def same(got, want, what=""):
    for name, g, w in zip(("results", "exons", "steps"), got, want):
        assert len(g) == len(w), (what, name, len(g), len(w))
        if g.tobytes() != w.tobytes():
            bad = [i for i in range(len(g)) if g[i] != w[i]]
            raise AssertionError("%s: %s differ at %d places, first %d: %r / %r" % (what, name, len(bad), bad[0], g[bad[0]], w[bad[0]]))


def device(idx, ests, exons, q, prm):
    return idx.factorizations(ests, exons, q, *prm)


@pytest.fixture(scope="module")
def indexes(gpu_ctx):
    """one index per fixture sequence, and one over the hand-made cases' sequence"""
    import pintron_amd.capi as capi
    seqs = {name: F.fixture_groups(name)[0] for name in FIXTURES}
    seqs["hand"] = F.hand_sequence()
    idx = {name: capi.Index(gpu_ctx, g) for name, g in seqs.items()}
    yield seqs, idx
    for i in idx.values():
        i.close()


COVER = {"clean_chains": (1110, 446, 0), "gap_chains": (1120, 852, 0), "refine_chains": (1119, 360, 3)}      # cases, DONE, dropped_first


@pytest.mark.parametrize("name", FIXTURES)
def test_index_form_against_the_restatement_twice_and_on_a_loaded_index(indexes, gpu_ctx, tmp_path, name):
    import pintron_amd.capi as capi
    seqs, idx = indexes
    gen, groups = F.fixture_groups(name)
    answers = F.fixture_answers(name)
    path = str(tmp_path / (name + ".idx"))
    idx[name].save(path)
    loaded = capi.Index(gpu_ctx, gen, load_from=path)
    try:
        n_cases = n_done = n_dropped = 0
        for prm, cases in groups.items():                        # every group: built, a second time, reloaded
            ests, exons, q = F.batch_arrays(cases)
            want = F.expect_arrays(answers[prm])
            first = device(idx[name], ests, exons, q, prm)
            same(first, want, (name, prm))
            assert idx[name].factorizations_kernel_ms() > 0.0
            again = device(idx[name], ests, exons, q, prm)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(first, again))
            same(device(loaded, ests, exons, q, prm), want, (name, prm, "loaded"))
            done = first[0]["outcome"] == F.DONE
            n_cases, n_done, n_dropped = n_cases + len(cases), n_done + int(done.sum()), n_dropped + int((first[0]["detail"][done] & 1).sum())
        assert (n_cases, n_done, n_dropped) == COVER[name]
    finally:
        loaded.close()


@pytest.mark.parametrize("name", FIXTURES)
def test_index_form_against_the_call_by_call_route(indexes, name):
    seqs, idx = indexes
    n_cases = n_done = n_dropped = 0
    for prm, cases in F.fixture_groups(name)[1].items():         # every group, the 394 settings of refine_chains too
        ests, exons, q = F.batch_arrays(cases)
        route = F.call_by_call(idx[name], len(seqs[name]), ests, exons, q, prm)
        same(device(idx[name], ests, exons, q, prm), route, (name, prm))
        done = route[0]["outcome"] == F.DONE
        n_cases, n_done, n_dropped = n_cases + len(cases), n_done + int(done.sum()), n_dropped + int((route[0]["detail"][done] & 1).sum())
    assert (n_cases, n_done, n_dropped) == COVER[name]


def hand_batches():
    g, cases = F.hand_cases()
    by_prm = {}
    for name, est, ex, prm, want in cases:
        by_prm.setdefault(prm, []).append((name, est, ex, want))
    return g, by_prm


def test_hand_made_cases_against_the_restatement_and_the_route(indexes):
    seqs, idx = indexes
    g, by_prm = hand_batches()
    seen = set()
    for prm, cases in by_prm.items():
        ests, exons, q = F.batch_arrays([(est, ex) for _, est, ex, _ in cases])
        want = F.expect_arrays([F.factorization(KL.ONE if ex else KL.NONE, est, g, ex, prm) for _, est, ex, _ in cases])
        got = device(idx["hand"], ests, exons, q, prm)
        same(got, want, prm)
        same(got, F.call_by_call(idx["hand"], len(g), ests, exons, q, prm), (prm, "route"))
        for (name, _, _, claim), r in zip(cases, got[0]):
            cell = (int(r["outcome"]), int(r["stage"]), int(r["detail"]))
            if claim is not None:
                assert cell[:2] == claim[:2] and (claim[2] is None or cell[2] == claim[2]), (name, cell)
            seen.add(cell)
    assert {(F.HOST, 0, KL.NONE), (F.HOST, 1, 1), (F.HOST, 1, 2), (F.HOST, 2, 1), (F.HOST, 2, 2), (F.HOST, 3, 1)} <= seen
    assert (F.HOST, 3, 2) not in seen                           # nothing reaches it


def test_a_host_outcome_in_the_middle_leaves_its_neighbours_alone(indexes):
    """a batch of DONE queries with one query HOST at each stage in its middle: no placeholder leaks into a neighbour"""
    seqs, idx = indexes
    g, by_prm = hand_batches()
    cases = {name: (est, ex) for name, est, ex, _ in by_prm[F.DEFAULTS]}
    done = [cases["plain"], cases["exons_64"], cases["est_gap_64"], cases["gap_p_equals_gap_t"]]
    alone = {}
    for k, c in enumerate(done):
        ests, exons, q = F.batch_arrays([c])
        alone[k] = device(idx["hand"], ests, exons, q, F.DEFAULTS)
        assert alone[k][0]["outcome"][0] == F.DONE
    for bad in ("no_candidate", "exons_65", "coordinate_outside", "est_gap_65", "gap_p_above_gap_t", "exons_overlap_by_one"):
        batch = done[:2] + [cases[bad]] + done[2:]
        ests, exons, q = F.batch_arrays(batch)
        res, ex, st = device(idx["hand"], ests, exons, q, F.DEFAULTS)
        assert res["outcome"][2] == F.HOST and not res["n_exons"][2] and not res["first_exon"][2], bad
        for k, at in ((0, 0), (1, 1), (2, 3), (3, 4)):
            r1, e1, s1 = alone[k]
            lo, n = int(res["first_exon"][at]), int(res["n_exons"][at])
            assert (res["outcome"][at], n, res["n_merged"][at], res["total_edit"][at]) == \
                (F.DONE, r1["n_exons"][0], r1["n_merged"][0], r1["total_edit"][0]), (bad, k)
            assert ex[lo:lo + n].tobytes() == e1.tobytes() and st[lo:lo + n].tobytes() == s1.tobytes(), (bad, k)
        assert int(res["n_exons"].sum()) == len(ex) == len(st)
    # HOST at stage 3 needs other settings than the defaults: under each, the query that meets refine's cap between DONE
    # neighbours, which are compared with a run of each alone under the same settings.  What must not leak: the placeholders
    # of the hand-off in front of refine, the exons chain_kernel wrote before it refused, the gather's counts and offsets
    wide = {name: (est, ex) for prm_, cs in by_prm.items() for name, est, ex, _ in cs if name.startswith(("est_window", "gen_window"))}
    for bad, prm in (("est_window_193", (20.0, 97, 30, 30, 40)), ("gen_window_321", (20.0, 30, 64, 97, 40))):
        done3 = [cases["plain"], cases["exons_64"], cases["exons_64"], cases["plain"]]      # DONE under both settings
        alone3 = []
        for c in done3:
            ests, exons, q = F.batch_arrays([c])
            alone3.append(device(idx["hand"], ests, exons, q, prm))
            assert alone3[-1][0]["outcome"][0] == F.DONE, (bad, prm)
        batch = done3[:2] + [wide[bad]] + done3[2:]
        ests, exons, q = F.batch_arrays(batch)
        res, ex, st = device(idx["hand"], ests, exons, q, prm)
        assert (res["outcome"][2], res["stage"][2], res["detail"][2]) == (F.HOST, 3, 1), bad
        assert not res["n_exons"][2] and not res["first_exon"][2] and not res["n_merged"][2]
        for k, at in ((0, 0), (1, 1), (2, 3), (3, 4)):
            r1, e1, s1 = alone3[k]
            lo, n = int(res["first_exon"][at]), int(res["n_exons"][at])
            assert (res["outcome"][at], n, res["n_merged"][at], res["total_edit"][at]) == \
                (F.DONE, r1["n_exons"][0], r1["n_merged"][0], r1["total_edit"][0]), (bad, k)
            assert ex[lo:lo + n].tobytes() == e1.tobytes() and st[lo:lo + n].tobytes() == s1.tobytes(), (bad, k)
        assert int(res["n_exons"].sum()) == len(ex) == len(st)
        same((res, ex, st), F.expect_arrays([F.factorization(KL.ONE, e_, g, x_, prm) for e_, x_ in batch]), bad)
    # 65 queries, every third without a candidate: an odd count whose last EST has the most work
    batch = [done[k % 2 * 3] if k % 3 else cases["no_candidate"] for k in range(64)] + [cases["exons_64"]]
    ests, exons, q = F.batch_arrays(batch)
    got = device(idx["hand"], ests, exons, q, F.DEFAULTS)
    same(got, F.expect_arrays([F.factorization(KL.ONE if ex else KL.NONE, est, g, ex) for est, ex in batch]))
    assert got[0]["outcome"][64] == F.DONE and got[0]["n_exons"][64] == 64


# ---- the plan form ------------------------------------------------------------------------------------------------
def run_plan(plan, prm, fprm=F.DEFAULTS, rate=0.2):
    plan.run(prm["min_factor_len"], rate)
    plan.run_meg(**prm)
    plan.run_candidates(prm["min_factor_len"], prm["min_intron_length"])
    plan.run_factorizations(*fprm)
    return plan.fetch_factorizations()


def restated(seqs, genomic, cand, ks, fprm=F.DEFAULTS):
    """the restatement on the candidates the device fetched, for the ESTs `ks`"""
    res, ex = cand
    out = {}
    for k in ks:
        first, n = int(res["first_exon"][k]), int(res["n_exons"][k])
        out[k] = F.factorization(int(res["kind"][k]), seqs[k], genomic, [tuple(int(v) for v in e) for e in ex[first:first + n]], fprm)
    return out


def sub_results(got, ks):
    """the results, exons and steps of the ESTs `ks` of a call, as a call of their own"""
    res, ex, st = got
    sub = res[ks].copy()
    exs, sts, at = [], [], 0
    for j, k in enumerate(ks):
        if res["outcome"][k] == F.DONE:
            lo, n = int(res["first_exon"][k]), int(res["n_exons"][k])
            exs.append(ex[lo:lo + n])
            sts.append(st[lo:lo + n])
            sub["first_exon"][j] = at
            at += n
    return (sub, np.concatenate(exs) if exs else ex[:0], np.concatenate(sts) if sts else st[:0])


@pytest.mark.parametrize("source,n_pat", [("c2", 307), ("issue13", 1891)])
@pytest.mark.parametrize("resident", [False, True])
def test_plan_form_against_the_restatement_the_index_form_and_the_route(gpu_ctx, source, n_pat, resident):
    import pintron_amd.capi as capi
    gfa, efa = KL.real_inputs()[source]
    prm = M.DEFAULTS
    exp, genomic = M.first_attempt_megs(gfa, efa, prm)
    seqs = [e["seq"] for e in exp]
    assert len(seqs) == n_pat
    idx = capi.Index(gpu_ctx, genomic)
    plan = capi.PairingPlan(gpu_ctx, idx, seqs, resident=resident)
    try:
        got = run_plan(plan, prm)
        assert all(plan.factorizations_ms(k) > 0.0 for k in range(4))
        assert plan.factorizations_ms(0) >= plan.factorizations_ms(1) + plan.factorizations_ms(2) + plan.factorizations_ms(3)
        cand = plan.fetch_candidates()
        res = got[0]
        # the restatement on the device's own candidates: every pattern of c2, a fixed-seed sample of 200 of issue13
        ks = list(range(n_pat)) if n_pat <= 400 else sorted(np.random.default_rng(13).choice(n_pat, 200, replace=False).tolist())
        mine = restated(seqs, genomic, cand, ks)
        same(sub_results(got, ks), F.expect_arrays([mine[k] for k in ks]), source)
        # ... and from the device's own fetched records: record -> cand_lib.candidate -> the restatement
        recs = plan.fetch_meg()
        L, mi = prm["min_factor_len"], prm["min_intron_length"]
        from_recs = []
        for k in ks:
            kind, _, _, cex = KL.candidate(recs[k], genomic, L, mi)
            from_recs.append(F.factorization(kind, seqs[k], genomic, cex, F.DEFAULTS))
        same(sub_results(got, ks), F.expect_arrays(from_recs), source + " from the records")
        # the index form fed with the fetched candidates, and the call-by-call route: byte for byte, every pattern
        off = np.zeros(n_pat + 1, dtype=np.uint64)
        np.cumsum([len(s) for s in seqs], out=off[1:])
        q = F.plan_queries(off, cand[0])
        blob = b"".join(seqs)
        r2, e2, s2 = device(idx, blob, cand[1], q, F.DEFAULTS)
        same(got, (F.stage0_of_kinds(r2, cand[0]["kind"]), e2, s2), source + " index form")
        r3, e3, s3 = F.call_by_call(idx, len(genomic), blob, cand[1], q, F.DEFAULTS)
        same(got, (F.stage0_of_kinds(r3, cand[0]["kind"]), e3, s3), source + " route")
        # the cover
        done = res["outcome"] == F.DONE
        assert done.sum() > n_pat // 4, done.sum()
        assert (res["outcome"][cand[0]["kind"] == KL.NOT_PATH] == F.HOST).all() and (cand[0]["kind"] == KL.NOT_PATH).any()
        assert (res["outcome"] == F.EMPTY).any()
        if source == "issue13":
            at_clean = res[(res["outcome"] == F.EMPTY) & (res["stage"] == 1)]
            assert {4, 6, 7} <= set(int(d) for d in at_clean["detail"]) and len(at_clean) >= 25
            assert (res["n_merged"][done] > 0).any() and ((res["outcome"] == F.EMPTY) & (res["stage"] == 0)).any()
            assert not ((res["outcome"] == F.HOST) & (res["stage"] > 0)).any()
        # a rerun, other parameters and back: the same bytes; the candidates stay what they were
        again = run_plan(plan, prm)
        other = (2.0, 20, 40, 20, 60)
        got2 = run_plan(plan, prm, other)
        ks2 = ks[:60]
        same(sub_results(got2, ks2), F.expect_arrays([restated(seqs, genomic, cand, ks2, other)[k] for k in ks2]), source + " other")
        plan.run_factorizations(*F.DEFAULTS)                           # without a new run_candidates
        back = plan.fetch_factorizations()
        for g in (again, back):
            assert all(a.tobytes() == b.tobytes() for a, b in zip(g, got))
        after = plan.fetch_candidates()
        assert after[0].tobytes() == cand[0].tobytes() and after[1].tobytes() == cand[1].tobytes()
    finally:
        plan.close()
        idx.close()


def test_without_timing_the_answers_are_the_same(indexes):
    import pintron_amd.capi as capi
    seqs, _ = indexes
    g, by_prm = hand_batches()
    cases = [(est, ex) for _, est, ex, _ in by_prm[F.DEFAULTS]]
    ests, exons, q = F.batch_arrays(cases)
    want = F.expect_arrays([F.factorization(KL.ONE if ex else KL.NONE, est, g, ex) for est, ex in cases])
    gfa, efa = M.rerun_input()
    exp, genomic = M.first_attempt_megs(gfa, efa)
    with capi.Context(0) as ctx:
        idx = capi.Index(ctx, g)
        same(device(idx, ests, exons, q, F.DEFAULTS), want)
        assert idx.factorizations_kernel_ms() > 0.0
        ctx.L.pgpu_set_timing(ctx.h, 0)
        same(device(idx, ests, exons, q, F.DEFAULTS), want)
        assert idx.factorizations_kernel_ms() == 0.0
        idx.close()
        ctx.L.pgpu_set_timing(ctx.h, 1)
        idx = capi.Index(ctx, genomic)
        seqs_ = [e["seq"] for e in exp]
        plan = capi.PairingPlan(ctx, idx, seqs_)
        timed = run_plan(plan, M.DEFAULTS)
        assert all(plan.factorizations_ms(k) > 0.0 for k in range(4))
        plan.close()
        ctx.L.pgpu_set_timing(ctx.h, 0)
        plan = capi.PairingPlan(ctx, idx, seqs_)                   # made with timing off: it has no events
        got = run_plan(plan, M.DEFAULTS)
        assert all(plan.factorizations_ms(k) == 0.0 for k in range(4))
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, timed))
        plan.close()
        idx.close()


# ---- refusals -----------------------------------------------------------------------------------------------------
def test_refusals_of_the_plan_form(gpu_ctx):
    import pintron_amd.capi as capi
    L_ = gpu_ctx.L
    gfa, efa = M.rerun_input()
    exp, genomic = M.first_attempt_megs(gfa, efa)
    seqs = [e["seq"] for e in exp]
    idx = capi.Index(gpu_ctx, genomic)
    plan = capi.PairingPlan(gpu_ctx, idx, seqs)
    res = np.zeros(len(seqs), dtype=np.dtype(capi.FACT_RESULT_DTYPE))
    ex = np.zeros(4096, dtype=np.dtype(capi.FACTOR_DTYPE))
    st = np.zeros(4096, dtype=np.uint8)
    rp, ep, sp = res.ctypes.data_as(C.POINTER(capi.FactResult)), ex.ctypes.data_as(C.POINTER(capi.Factor)), st.ctypes.data_as(C.POINTER(C.c_uint8))

    def run_f(fprm=F.DEFAULTS, p=None):
        prm = capi.FactParams(*fprm)
        return L_.pgpu_pairing_plan_run_factorizations(gpu_ctx.h, (p or plan).h, C.byref(prm))

    def fetch(cap=4096, p=None):
        return L_.pgpu_pairing_plan_fetch_factorizations(gpu_ctx.h, (p or plan).h, rp, ep, sp, cap)

    def message():
        return L_.pgpu_last_error(gpu_ctx.h).decode()
    try:
        assert fetch() == capi.PGPU_EINVAL and "run_factorizations first" in message()      # nothing ran yet
        assert run_f() == capi.PGPU_EINVAL and "run_candidates" in message()
        plan.run(15, 0.2)
        plan.run_meg(**M.DEFAULTS)
        assert run_f() == capi.PGPU_EINVAL and "run_candidates" in message()                 # records, no candidates
        plan.run_candidates(15, 40)
        for bad in ((20.0, -1, 70, 30, 40), (20.0, 30, (1 << 24) + 1, 30, 40), (20.0, 30, 70, -5, 40)):
            assert run_f(bad) == capi.PGPU_EINVAL and message() == BAD_PARAMS
            assert fetch() == capi.PGPU_EINVAL                                               # a refused run leaves nothing to fetch
            assert L_.pgpu_pairing_plan_factorization_exons(plan.h) == 0 and plan.factorizations_ms(0) == 0.0
        assert run_f((20.0, 0, 1 << 24, 30, -7)) == capi.PGPU_OK                             # the bounds themselves, any min_intron_length
        assert run_f() == capi.PGPU_OK
        n = L_.pgpu_pairing_plan_factorization_exons(plan.h)
        assert n > 0 and plan.factorizations_ms(0) > 0.0
        assert fetch(n - 1) == capi.PGPU_ENOSPC and fetch(0) == capi.PGPU_ENOSPC and message() == "exon buffer too small"
        assert fetch(n) == capi.PGPU_OK
        want = (res.copy(), ex[:n].copy(), st[:n].copy())
        assert int(want[0]["n_exons"].sum()) == n
        assert L_.pgpu_pairing_plan_run_factorizations(gpu_ctx.h, plan.h, None) == capi.PGPU_EINVAL
        assert L_.pgpu_pairing_plan_run_factorizations(gpu_ctx.h, None, C.byref(capi.FactParams(*F.DEFAULTS))) == capi.PGPU_EINVAL
        assert L_.pgpu_pairing_plan_fetch_factorizations(gpu_ctx.h, plan.h, None, ep, sp, 4096) == capi.PGPU_EINVAL
        assert L_.pgpu_pairing_plan_fetch_factorizations(gpu_ctx.h, plan.h, rp, ep, None, 4096) == capi.PGPU_EINVAL
        assert L_.pgpu_pairing_plan_factorization_exons(None) == 0 and L_.pgpu_pairing_plan_factorizations_ms(None, 0) == 0.0
        assert plan.factorizations_ms(4) == 0.0 and plan.factorizations_ms(-1) == 0.0
        assert run_f() == capi.PGPU_OK and fetch(n) == capi.PGPU_OK
        assert (res.tobytes(), ex[:n].tobytes(), st[:n].tobytes()) == tuple(w.tobytes() for w in want)
        plan.run_candidates(15, 40)                                                          # new candidates: the answer is gone
        assert fetch(n) == capi.PGPU_EINVAL and "run_factorizations first" in message()
        plan.run_meg(**M.DEFAULTS)                                                           # new records: the candidates are gone
        assert run_f() == capi.PGPU_EINVAL and "run_candidates" in message()
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
            p.run_factorizations(*F.DEFAULTS)
        assert fetch(p=a) == capi.PGPU_EINVAL and "overwritten" in message()
        assert run_f(p=a) == capi.PGPU_EINVAL and "overwritten" in message()
        assert fetch(p=a) == capi.PGPU_EINVAL and "run_factorizations first" in message()    # a refused run leaves nothing to fetch
        got_b = b.fetch_factorizations()
        whole = capi.PairingPlan(gpu_ctx, idx, seqs[30:])
        try:
            same(got_b, run_plan(whole, M.DEFAULTS), "resident against plain")
        finally:
            whole.close()
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
            assert plan.run_candidates(15, 40) == 0
            assert plan.run_factorizations(*F.DEFAULTS) == 0 and plan.factorizations_ms(0) == 0.0
            assert gpu_ctx.L.pgpu_pairing_plan_fetch_factorizations(gpu_ctx.h, plan.h, None, None, None, 0) == capi.PGPU_OK
        finally:
            plan.close()
    idx.close()


def test_refusals_and_the_contract_of_the_index_form(indexes, gpu_ctx):
    import pintron_amd.capi as capi
    L_ = gpu_ctx.L
    seqs, idxs = indexes
    g, idx = seqs["hand"], idxs["hand"]
    _, by_prm = hand_batches()
    cases = [(est, ex) for _, est, ex, _ in by_prm[F.DEFAULTS]]
    ests, exons, q = F.batch_arrays(cases)
    want = F.expect_arrays([F.factorization(KL.ONE if ex else KL.NONE, est, g, ex) for est, ex in cases])
    n, n_out = len(q), len(want[1])
    assert n_out > 60
    f = L_.pgpu_index_factorizations

    def raw(q_, fprm=F.DEFAULTS, cap=None, ests_len=None, n_ex=None):
        """the call with its outputs filled beforehand -> (rc, whether anything was written, *n_out, outputs)"""
        cap = n_out if cap is None else cap
        res = np.full(16 * max(len(q_), 1), 0x55, dtype=np.uint8).view(np.dtype(capi.FACT_RESULT_DTYPE))
        ex = np.full(16 * max(cap, 1), 0x55, dtype=np.uint8).view(np.dtype(capi.FACTOR_DTYPE))
        st = np.full(max(cap, 1), 0x55, dtype=np.uint8)
        total = C.c_size_t(12345)
        prm = capi.FactParams(*fprm)
        rc = f(gpu_ctx.h, idx.h, ests, len(ests) if ests_len is None else ests_len, exons.ctypes.data_as(C.POINTER(capi.Factor)),
               len(exons) if n_ex is None else n_ex, q_.ctypes.data_as(C.POINTER(capi.FactQuery)), len(q_), C.byref(prm),
               res.ctypes.data_as(C.POINTER(capi.FactResult)), ex.ctypes.data_as(C.POINTER(capi.Factor)),
               st.ctypes.data_as(C.POINTER(C.c_uint8)), cap, C.byref(total))
        untouched = all((x.view(np.uint8) == 0x55).all() for x in (res, ex, st))
        return rc, untouched, total.value, (res, ex, st)

    def good():
        rc, _, total, (res, ex, st) = raw(q)
        assert rc == capi.PGPU_OK and total == n_out
        same((res, ex[:n_out], st[:n_out]), want)
        assert idx.factorizations_kernel_ms() > 0.0

    def refused(q_, message=BAD_QUERY, **kw):
        good()                                                                   # a slot for the refusal to reset
        rc, untouched, total, _ = raw(q_, **kw)
        assert rc == capi.PGPU_EINVAL and untouched and total == 12345
        assert L_.pgpu_last_error(gpu_ctx.h).decode() == message and idx.factorizations_kernel_ms() == 0.0

    for bad in ((20.0, -1, 70, 30, 40), (20.0, 30, (1 << 24) + 1, 30, 40), (20.0, 30, 70, 1 << 30, 40)):
        refused(q, message=BAD_PARAMS, fprm=bad)
    refused(q, ests_len=len(ests) - 1)                                           # the last EST runs past the buffer
    refused(q, n_ex=len(exons) - 1)                                              # the last candidate past the exons
    mid = next(k for k in range(3, n) if q["n_exons"][k])
    for field, value in (("reserved", 1), ("est_len", 0), ("est_off", len(ests)), ("est_len", len(ests) + 1),
                         ("first_exon", len(exons)), ("n_exons", len(exons) + 1), ("first_exon", int(q["first_exon"][mid]) - 1)):
        q2 = q.copy()
        q2[field][mid] = value
        refused(q2)
    # the values of the exons are no refusal: a candidate of garbage is HOST for itself, its neighbours are untouched
    ex_keep = exons.copy()
    try:
        lo = int(q["first_exon"][mid])
        exons[lo] = (-2, 5, 1 << 30, -(1 << 31))
        rc, _, total, (res, _, _) = raw(q)
        assert rc == capi.PGPU_OK and (res["outcome"][mid], res["stage"][mid], res["detail"][mid]) == (F.HOST, 1, 2)
        others = [k for k in range(n) if k != mid]
        assert (res["outcome"][others] == want[0]["outcome"][others]).all() and (res["n_exons"][others] == want[0]["n_exons"][others]).all()
    finally:
        exons[:] = ex_keep
    # PGPU_ENOSPC: the count, and nothing written
    for cap in (0, n_out - 1):
        good()
        rc, untouched, total, _ = raw(q, cap=cap)
        assert rc == capi.PGPU_ENOSPC and untouched and total == n_out and idx.factorizations_kernel_ms() == 0.0
        assert L_.pgpu_last_error(gpu_ctx.h).decode() == "exon buffer too small"
    # null pointers: a bare refusal, the message stays
    good()
    raw(q, fprm=(20.0, -1, 70, 30, 40))
    res = np.zeros(n, dtype=np.dtype(capi.FACT_RESULT_DTYPE))
    ex = np.zeros(n_out, dtype=np.dtype(capi.FACTOR_DTYPE))
    st = np.zeros(n_out, dtype=np.uint8)
    total = C.c_size_t(0)
    prm = capi.FactParams(*F.DEFAULTS)
    full = [gpu_ctx.h, idx.h, ests, len(ests), exons.ctypes.data_as(C.POINTER(capi.Factor)), len(exons),
            q.ctypes.data_as(C.POINTER(capi.FactQuery)), n, C.byref(prm), res.ctypes.data_as(C.POINTER(capi.FactResult)),
            ex.ctypes.data_as(C.POINTER(capi.Factor)), st.ctypes.data_as(C.POINTER(C.c_uint8)), n_out, C.byref(total)]
    for k in (0, 1, 2, 4, 6, 8, 9, 10, 11, 13):
        args = list(full)
        args[k] = None
        assert f(*args) == capi.PGPU_EINVAL, k
        if k:
            assert L_.pgpu_last_error(gpu_ctx.h).decode() == BAD_PARAMS and idx.factorizations_kernel_ms() == 0.0
    # n == 0, and a batch without a candidate: no exon, no buffer needed
    good()
    total.value = 99
    assert f(gpu_ctx.h, idx.h, None, 0, None, 0, None, 0, C.byref(prm), None, None, None, 0, C.byref(total)) == capi.PGPU_OK
    assert total.value == 0 and idx.factorizations_kernel_ms() == 0.0
    q0 = np.zeros(2, dtype=np.dtype(capi.FACT_QUERY_DTYPE))
    q0["est_len"] = 10
    q0["first_exon"] = 1 << 30                                                   # not looked at
    total.value = 99
    assert f(gpu_ctx.h, idx.h, ests, len(ests), None, 0, q0.ctypes.data_as(C.POINTER(capi.FactQuery)), 2, C.byref(prm),
             res.ctypes.data_as(C.POINTER(capi.FactResult)), None, None, 0, C.byref(total)) == capi.PGPU_OK
    assert total.value == 0 and [tuple(int(v) for v in r)[:3] for r in res[:2]] == [(F.HOST, 0, KL.NONE)] * 2
    good()                                                                       # the context still answers
