"""GPU: the final stage -- pgpu_index_final_factorizations and pgpu_pairing_plan_run_final_factorizations against the
restatement (tests/final_lib.py) and against today's route (pgpu_index_factorizations, pgpu_index_tail_chains and
pgpu_index_small_chains called one after the other with the glue on the host).  Every comparison is byte equality:
results, exons, step bytes."""
import ctypes as C

import numpy as np
import pytest

import cand_lib as KL
import fact_lib as F
import final_lib as FL
import meg_lib as M
import small_lib as SL
import tail_lib as TL

pytestmark = pytest.mark.gpu

BAD_PARAMS = "bad factorization parameters (a suffpref length outside [0, 2^24])"
BAD_SMALL = "bad small-chains parameters (reserved != 0)"
BAD_QUERY = "bad final query (a range past its buffer, an empty EST, reserved != 0, or an exon two queries share)"


def same(got, want, what=""):
    for name, g, w in zip(("results", "exons", "steps"), got, want):
        assert len(g) == len(w), (what, name, len(g), len(w))
        if g.tobytes() != w.tobytes():
            bad = [i for i in range(len(g)) if g[i] != w[i]]
            raise AssertionError("%s: %s differ at %d places, first %d: %r / %r" % (what, name, len(bad), bad[0], g[bad[0]], w[bad[0]]))


def device(idx, ests, exons, q, prm, mil):
    import pintron_amd.capi as capi
    rc, res, ex, st, total = idx.final_factorizations_raw(ests, exons, q, len(q), capi.FactParams(*prm), capi.SmallParams(mil, 0),
                                                          2 * len(exons))
    idx.ctx.check(rc)
    return res, ex[:total], st[:total]


def triples(cases):
    return [(c["orig"], c["est"], c["exons"]) for c in cases]


def restated(cases, g, prm, mil, ops=None):
    return [FL.final(KL.ONE if c["exons"] else KL.NONE, c["orig"], c["est"], g, c["exons"], prm, mil, ops=ops) for c in cases]


# ---- the index form ---------------------------------------------------------------------------------------------------
def test_hand_made_cases_against_the_restatement_and_the_route_built_reloaded_and_twice(gpu_ctx, tmp_path):
    import pintron_amd.capi as capi
    seen = set()
    for name, g, cases in FL.hand_groups():
        idx = capi.Index(gpu_ctx, g)
        path = str(tmp_path / (name + ".idx"))
        idx.save(path)
        loaded = capi.Index(gpu_ctx, g, load_from=path)
        try:
            for (prm, mil), group in FL.by_settings(cases).items():
                ests, exons, q = FL.batch_arrays(triples(group))
                want = FL.expect_arrays([c["answer"] for c in group])
                first = device(idx, ests, exons, q, prm, mil)
                same(first, want, (name, prm, mil))
                assert idx.final_factorizations_kernel_ms() > 0.0
                again = device(idx, ests, exons, q, prm, mil)
                assert all(a.tobytes() == b.tobytes() for a, b in zip(first, again))
                same(device(loaded, ests, exons, q, prm, mil), want, (name, prm, mil, "loaded"))
                same(first, FL.route(idx, len(g), ests, exons, q, prm, mil), (name, prm, mil, "route"))
                for c in group:
                    seen |= c["tags"]
        finally:
            loaded.close()
            idx.close()
    assert seen == set(FL.TAGS) - set(FL.NOT_REACHED), sorted(set(FL.TAGS) - set(FL.NOT_REACHED) - seen)


def _fixture_cases(name):
    """(sequence, {(prm, mil): [case dicts]}) of one of the five chained fixtures, its lists as candidates"""
    if name in ("clean_chains", "gap_chains", "refine_chains"):
        g, groups = F.fixture_groups(name)
        return g, {(prm, int(prm[4])): [dict(orig=est, est=est, exons=ex) for est, ex in cases] for prm, cases in groups.items()}
    if name == "tail_chains":
        g, cases, _ = TL.load_fixture()
        return g, {(F.DEFAULTS, int(F.DEFAULTS[4])): [dict(orig=c["orig"], est=c["est"], exons=c["exons"]) for c in cases]}
    g, cases = SL.load_fixture()[0][0]
    out = {}
    for c in cases:
        out.setdefault((F.DEFAULTS[:4] + (c["mil"],), c["mil"]), []).append(dict(orig=c["orig"], est=c["est"], exons=c["exons"]))
    return g, out


@pytest.mark.parametrize("name", ["clean_chains", "gap_chains", "refine_chains", "tail_chains", "small_chains"])
def test_the_chained_fixtures_lists_as_candidates(gpu_ctx, name):
    import pintron_amd.capi as capi
    g, groups = _fixture_cases(name)
    idx = capi.Index(gpu_ctx, g)
    ops = SL.OracleOps(g)
    try:
        n_cases = n_done = 0
        for (prm, mil), cases in groups.items():
            ests, exons, q = FL.batch_arrays(triples(cases))
            got = device(idx, ests, exons, q, prm, mil)
            same(got, FL.route(idx, len(g), ests, exons, q, prm, mil), (name, prm, mil, "route"))
            same(got, FL.expect_arrays(restated(cases, g, prm, mil, ops)), (name, prm, mil))
            n_cases, n_done = n_cases + len(cases), n_done + int((got[0]["outcome"] == FL.DONE).sum())
            assert len(got[1]) <= 2 * len(exons)
        assert n_cases >= 250 and n_done >= 100, (n_cases, n_done)
    finally:
        idx.close()


@pytest.fixture(scope="module")
def hand(gpu_ctx):
    """the hand-made cases over the tail fixture's sequence under the defaults, their index and their arrays"""
    import pintron_amd.capi as capi
    name, g, cases = FL.hand_groups()[0]
    cases = FL.by_settings(cases)[(F.DEFAULTS, int(F.DEFAULTS[4]))]
    idx = capi.Index(gpu_ctx, g)
    yield g, idx, cases
    idx.close()


def test_batches_of_1_255_256_and_257_queries(hand):
    g, idx, cases = hand
    prm, mil = F.DEFAULTS, int(F.DEFAULTS[4])
    for n in (1, 255, 256, 257):
        batch = [cases[(7 * k) % len(cases)] for k in range(n)]
        ests, exons, q = FL.batch_arrays(triples(batch))
        same(device(idx, ests, exons, q, prm, mil), FL.expect_arrays([c["answer"] for c in batch]), n)


def test_a_batch_without_a_done_est_and_a_host_query_between_done_neighbours(hand):
    g, idx, cases = hand
    prm, mil = F.DEFAULTS, int(F.DEFAULTS[4])
    done = [c for c in cases if c["answer"]["outcome"] == FL.DONE]
    rest = [c for c in cases if c["answer"]["outcome"] != FL.DONE]
    assert len(done) >= 4 and len(rest) >= 2
    none = dict(done[0], exons=None)
    batch = rest + [none]
    ests, exons, q = FL.batch_arrays(triples(batch))
    res, ex, st = device(idx, ests, exons, q, prm, mil)
    same((res, ex, st), FL.expect_arrays([c["answer"] for c in rest] + [FL.final(KL.NONE, none["orig"], none["est"], g, None)]))
    assert len(ex) == 0 and not (res["outcome"] == FL.DONE).any()
    alone = []
    for c in done[:4]:
        ests, exons, q = FL.batch_arrays(triples([c]))
        alone.append(device(idx, ests, exons, q, prm, mil))
    for bad in rest + [none]:
        batch = done[:2] + [bad] + done[2:4]
        ests, exons, q = FL.batch_arrays(triples(batch))
        res, ex, st = device(idx, ests, exons, q, prm, mil)
        assert res["outcome"][2] != FL.DONE and not res["n_exons"][2] and not res["first_exon"][2]
        for k, at in ((0, 0), (1, 1), (2, 3), (3, 4)):
            r1, e1, s1 = alone[k]
            lo, n = int(res["first_exon"][at]), int(res["n_exons"][at])
            a, b = res[at:at + 1].copy(), r1.copy()
            a["first_exon"], b["first_exon"] = 0, 0
            assert a.tobytes() == b.tobytes(), (bad["name"], k)
            assert ex[lo:lo + n].tobytes() == e1.tobytes() and st[lo:lo + n].tobytes() == s1.tobytes(), (bad["name"], k)
        assert int(res["n_exons"].sum()) == len(ex) == len(st)


def test_without_timing_the_answers_are_the_same():
    import pintron_amd.capi as capi
    name, g, cases = FL.hand_groups()[0]
    cases = FL.by_settings(cases)[(F.DEFAULTS, int(F.DEFAULTS[4]))]
    ests, exons, q = FL.batch_arrays(triples(cases))
    want = FL.expect_arrays([c["answer"] for c in cases])
    with capi.Context(0) as ctx:
        idx = capi.Index(ctx, g)
        same(device(idx, ests, exons, q, F.DEFAULTS, 40), want)
        assert idx.final_factorizations_kernel_ms() > 0.0
        ctx.L.pgpu_set_timing(ctx.h, 0)
        same(device(idx, ests, exons, q, F.DEFAULTS, 40), want)
        assert idx.final_factorizations_kernel_ms() == 0.0
        idx.close()


def test_refusals_and_the_contract_of_the_index_form(hand, gpu_ctx):
    import pintron_amd.capi as capi
    L_ = gpu_ctx.L
    g, idx, cases = hand
    ests, exons, q = FL.batch_arrays(triples(cases))
    want = FL.expect_arrays([c["answer"] for c in cases])
    n, n_out = len(q), len(want[1])
    assert n_out > 30
    f = L_.pgpu_index_final_factorizations

    def raw(q_, fprm=F.DEFAULTS, sprm=(40, 0), cap=None, ests_len=None, n_ex=None):
        """the call with its outputs filled beforehand -> (rc, whether anything was written, *n_out, outputs)"""
        cap = n_out if cap is None else cap
        res = np.full(32 * max(len(q_), 1), 0x55, dtype=np.uint8).view(np.dtype(capi.FINAL_RESULT_DTYPE))
        ex = np.full(16 * max(cap, 1), 0x55, dtype=np.uint8).view(np.dtype(capi.FACTOR_DTYPE))
        st = np.full(max(cap, 1), 0x55, dtype=np.uint8)
        total = C.c_size_t(12345)
        prm, small = capi.FactParams(*fprm), capi.SmallParams(*sprm)
        rc = f(gpu_ctx.h, idx.h, ests, len(ests) if ests_len is None else ests_len, exons.ctypes.data_as(C.POINTER(capi.Factor)),
               len(exons) if n_ex is None else n_ex, q_.ctypes.data_as(C.POINTER(capi.FinalQuery)), len(q_), C.byref(prm), C.byref(small),
               res.ctypes.data_as(C.POINTER(capi.FinalResult)), ex.ctypes.data_as(C.POINTER(capi.Factor)),
               st.ctypes.data_as(C.POINTER(C.c_uint8)), cap, C.byref(total))
        untouched = all((x.view(np.uint8) == 0x55).all() for x in (res, ex, st))
        return rc, untouched, total.value, (res, ex, st)

    def good():
        rc, _, total, (res, ex, st) = raw(q)
        assert rc == capi.PGPU_OK and total == n_out
        same((res, ex[:n_out], st[:n_out]), want)
        assert idx.final_factorizations_kernel_ms() > 0.0

    def refused(q_, message=BAD_QUERY, **kw):
        good()                                                                   # a slot for the refusal to reset
        rc, untouched, total, _ = raw(q_, **kw)
        assert rc == capi.PGPU_EINVAL and untouched and total == 12345
        assert L_.pgpu_last_error(gpu_ctx.h).decode() == message and idx.final_factorizations_kernel_ms() == 0.0

    for bad in ((20.0, -1, 70, 30, 40), (20.0, 30, (1 << 24) + 1, 30, 40), (20.0, 30, 70, 1 << 30, 40)):
        refused(q, message=BAD_PARAMS, fprm=bad)
    refused(q, message=BAD_SMALL, sprm=(40, 1))
    refused(q, ests_len=len(ests) - 1)                                           # the last sequence runs past the buffer
    refused(q, n_ex=len(exons) - 1)                                              # the last candidate past the exons
    mid = next(k for k in range(3, n) if q["n_exons"][k])
    for field, value in (("reserved", 1), ("est_len", 0), ("est_off", len(ests)), ("est_len", len(ests) + 1),
                         ("first_exon", len(exons)), ("n_exons", len(exons) + 1), ("first_exon", int(q["first_exon"][mid]) - 1),
                         ("orig_off", len(ests) - int(q["est_len"][mid]) + 1), ("orig_off", (1 << 64) - 1)):
        q2 = q.copy()
        q2[field][mid] = value
        refused(q2)
    q2 = q.copy()
    q2["orig_off"][mid] = len(ests) - int(q["est_len"][mid])                     # the last place an original can lie
    assert raw(q2)[0] == capi.PGPU_OK
    # the values of the exons are no refusal: a candidate of garbage is HOST for itself, its neighbours are untouched
    ex_keep = exons.copy()
    try:
        lo = int(q["first_exon"][mid])
        exons[lo] = (-2, 5, 1 << 30, -(1 << 31))
        rc, _, total, (res, _, _) = raw(q)
        assert rc == capi.PGPU_OK and (res["outcome"][mid], res["stage"][mid], res["detail"][mid]) == (FL.HOST, 1, 2)
        others = [k for k in range(n) if k != mid]
        assert (res["outcome"][others] == want[0]["outcome"][others]).all() and (res["n_exons"][others] == want[0]["n_exons"][others]).all()
    finally:
        exons[:] = ex_keep
    # PGPU_ENOSPC: the count, and nothing written
    for cap in (0, n_out - 1):
        good()
        rc, untouched, total, _ = raw(q, cap=cap)
        assert rc == capi.PGPU_ENOSPC and untouched and total == n_out and idx.final_factorizations_kernel_ms() == 0.0
        assert L_.pgpu_last_error(gpu_ctx.h).decode() == "exon buffer too small"
    # null pointers: a bare refusal, the message stays
    good()
    raw(q, fprm=(20.0, -1, 70, 30, 40))
    res = np.zeros(n, dtype=np.dtype(capi.FINAL_RESULT_DTYPE))
    ex = np.zeros(n_out, dtype=np.dtype(capi.FACTOR_DTYPE))
    st = np.zeros(n_out, dtype=np.uint8)
    total = C.c_size_t(0)
    prm, small = capi.FactParams(*F.DEFAULTS), capi.SmallParams(40, 0)
    full = [gpu_ctx.h, idx.h, ests, len(ests), exons.ctypes.data_as(C.POINTER(capi.Factor)), len(exons),
            q.ctypes.data_as(C.POINTER(capi.FinalQuery)), n, C.byref(prm), C.byref(small), res.ctypes.data_as(C.POINTER(capi.FinalResult)),
            ex.ctypes.data_as(C.POINTER(capi.Factor)), st.ctypes.data_as(C.POINTER(C.c_uint8)), n_out, C.byref(total)]
    for k in (0, 1, 2, 4, 6, 8, 9, 10, 11, 12, 14):
        args = list(full)
        args[k] = None
        assert f(*args) == capi.PGPU_EINVAL, k
        if k:
            assert L_.pgpu_last_error(gpu_ctx.h).decode() == BAD_PARAMS and idx.final_factorizations_kernel_ms() == 0.0
    # n == 0, and a batch without a candidate: no exon, no buffer needed
    good()
    total.value = 99
    assert f(gpu_ctx.h, idx.h, None, 0, None, 0, None, 0, C.byref(prm), C.byref(small), None, None, None, 0, C.byref(total)) == capi.PGPU_OK
    assert total.value == 0 and idx.final_factorizations_kernel_ms() == 0.0
    q0 = np.zeros(2, dtype=np.dtype(capi.FINAL_QUERY_DTYPE))
    q0["est_len"] = 10
    q0["first_exon"] = 1 << 30                                                   # not looked at
    total.value = 99
    assert f(gpu_ctx.h, idx.h, ests, len(ests), None, 0, q0.ctypes.data_as(C.POINTER(capi.FinalQuery)), 2, C.byref(prm), C.byref(small),
             res.ctypes.data_as(C.POINTER(capi.FinalResult)), None, None, 0, C.byref(total)) == capi.PGPU_OK
    assert total.value == 0 and [tuple(int(v) for v in r)[:3] for r in res[:2]] == [(FL.HOST, 0, KL.NONE)] * 2
    good()                                                                       # the context still answers


# ---- the hand-off kernels over made-up stage results ------------------------------------------------------------------
def test_the_hand_off_kernels_over_stage_results_no_input_brings_through_the_stages(gpu_ctx):
    """65 exons, a coordinate equal to a length, verdict 1 of tail with its flags, every refusal code of small, a list tail
    emptied: final_lib.probe_cases through pgpu_final_handoffs_probe (no stage kernel runs), against the glue written in
    final_lib.probe_expect -- alone, all in one batch, and in reverse order"""
    import pintron_amd.capi as capi
    cases = FL.probe_cases()
    assert all(sum(t in c["tags"] for c in cases) >= FL.MIN_PER_TAG for t in FL.NOT_REACHED)
    for batch in (cases, cases[::-1], cases[:1], [c for c in cases if c["fact"][0] != FL.DONE]):
        a = FL.probe_arrays(batch)
        want, asked = FL.probe_expect(batch)
        rc, tq, sq, ex_sin, res, ex, st = capi.final_handoffs_probe(gpu_ctx, FL.PROBE_GEN_LEN, a["ests_len"], a["q"], a["fres"], a["fex"],
                                                                      a["tres"], a["tex"], a["tst"], a["sres"], a["sex"], a["sst"])
        gpu_ctx.check(rc)
        same((res, ex, st), want, len(batch))
        E = len(a["fex"])
        for i, c in enumerate(batch):
            assert int(sq["n_exons"][i]) == asked[i], i
            assert (tq["est_off"][i], tq["est_len"][i], tq["orig_off"][i]) == (a["q"]["est_off"][i], c["est_len"], a["q"]["orig_off"][i])
            if asked[i] == 1 and int(sq["first_exon"][i]) == E + i:                # the trivial query on the EST's own placeholder
                assert tuple(int(v) for v in ex_sin[E + i]) == (0, 0, 0, 0)
            else:                                                                  # the exons tail kept, moved down
                lo = int(sq["first_exon"][i])
                kept = [e for e, s_ in zip(c["tail_exons"], c["tail_steps"]) if s_ & 3 != TL.REMOVED]
                assert lo == int(a["fres"]["first_exon"][i]) and [tuple(int(v) for v in e) for e in ex_sin[lo:lo + asked[i]]] == kept, i
    # the probe checks the structure it relies on
    a = FL.probe_arrays(cases[:3])
    a["fres"]["first_exon"][1] = 0                                                 # two DONE ranges that share exons
    rc = capi.final_handoffs_probe(gpu_ctx, FL.PROBE_GEN_LEN, a["ests_len"], a["q"], a["fres"], a["fex"], a["tres"], a["tex"], a["tst"],
                                   a["sres"], a["sex"], a["sst"])[0]
    assert rc == capi.PGPU_EINVAL


# ---- the plan form ----------------------------------------------------------------------------------------------------
def run_plan(plan, prm, fprm=F.DEFAULTS, mil=40, rate=0.2):
    plan.run(prm["min_factor_len"], rate)
    plan.run_meg(**prm)
    plan.run_candidates(prm["min_factor_len"], prm["min_intron_length"])
    plan.run_factorizations(*fprm)
    plan.run_final_factorizations(mil)
    return plan.fetch_final_factorizations()


def sub_results(got, ks):
    """the results, exons and steps of the ESTs `ks` of a call, as a call of their own"""
    res, ex, st = got
    sub = res[ks].copy()
    exs, sts, at = [], [], 0
    for j, k in enumerate(ks):
        if res["outcome"][k] == FL.DONE:
            lo, n = int(res["first_exon"][k]), int(res["n_exons"][k])
            exs.append(ex[lo:lo + n])
            sts.append(st[lo:lo + n])
            sub["first_exon"][j] = at
            at += n
    return (sub, np.concatenate(exs) if exs else ex[:0], np.concatenate(sts) if sts else st[:0])


def with_a_polyA_tail(seq):
    """an original for a working sequence: the same bytes with the last twelve turned into a polyA and a byte behind it"""
    return seq[:-12] + b"AAAAAAAAAAAC" if len(seq) > 40 else seq


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
    ops = SL.OracleOps(genomic)
    try:
        got = run_plan(plan, prm)
        assert all(plan.final_ms(k) > 0.0 for k in range(3)) and plan.final_ms(0) >= plan.final_ms(1) + plan.final_ms(2)
        fact = plan.fetch_factorizations()
        cand = plan.fetch_candidates()
        # the restatement on the device's own candidates: every pattern
        ks = list(range(n_pat))
        cres, cex = cand
        mine = []
        for k in ks:
            lo, n = int(cres["first_exon"][k]), int(cres["n_exons"][k])
            mine.append(FL.final(int(cres["kind"][k]), seqs[k], seqs[k], genomic, [tuple(int(v) for v in e) for e in cex[lo:lo + n]], ops=ops))
        same(sub_results(got, ks), FL.expect_arrays(mine), source)
        # the index form fed with the fetched candidates, and the route from the plan's own factorizations: every pattern
        off = np.zeros(n_pat + 1, dtype=np.uint64)
        np.cumsum([len(s) for s in seqs], out=off[1:])
        q = FL.plan_queries(off, cres)
        blob = b"".join(seqs)
        r2, e2, s2 = device(idx, blob, cex, q, F.DEFAULTS, 40)
        same(got, (FL.stage0_of_kinds(r2, cres["kind"]), e2, s2), source + " index form")
        same(got, FL.glue(idx, len(genomic), blob, q, fact, 40), source + " route")
        done = got[0]["outcome"] == FL.DONE
        assert done.sum() > n_pat // 5, done.sum()
        # the factorizations are what they were, a rerun gives the same bytes, and so does a run of another plan in between
        assert all(a.tobytes() == b.tobytes() for a, b in zip(plan.fetch_factorizations(), fact))
        plan.run_final_factorizations(40)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(plan.fetch_final_factorizations(), got))
        other = capi.PairingPlan(gpu_ctx, idx, seqs[:40], resident=resident)
        try:
            got_other = run_plan(other, prm)
            if resident:
                rc = plan.fetch_final_factorizations_raw()[0]
                assert rc == capi.PGPU_EINVAL and "overwritten" in gpu_ctx.L.pgpu_last_error(gpu_ctx.h).decode()
                assert plan.run_final_factorizations_raw() == capi.PGPU_EINVAL
                assert "overwritten" in gpu_ctx.L.pgpu_last_error(gpu_ctx.h).decode()
            same(sub_results(run_plan(plan, prm), list(range(40))), got_other, source + " the other plan")
            assert all(a.tobytes() == b.tobytes() for a, b in zip(plan.fetch_final_factorizations(), got))
        finally:
            other.close()
        # another min_intron_length for small alone, and back
        got4 = (plan.run_final_factorizations(4), plan.fetch_final_factorizations())[1]
        ks2 = sorted(np.random.default_rng(13).choice(n_pat, 40, replace=False).tolist())      # (a sample: the other value)
        mine4 = []
        for k in ks2:
            lo, n = int(cres["first_exon"][k]), int(cres["n_exons"][k])
            mine4.append(FL.final(int(cres["kind"][k]), seqs[k], seqs[k], genomic, [tuple(int(v) for v in e) for e in cex[lo:lo + n]], mil=4, ops=ops))
        same(sub_results(got4, ks2), FL.expect_arrays(mine4), source + " mil 4")
    finally:
        plan.close()
        idx.close()


def test_a_plan_with_originals_differs_from_one_without_exactly_where_the_restatement_says(gpu_ctx):
    import pintron_amd.capi as capi
    gfa, efa = KL.real_inputs()["c2"]
    prm = M.DEFAULTS
    exp, genomic = M.first_attempt_megs(gfa, efa, prm)
    seqs = [e["seq"] for e in exp]
    n_pat = len(seqs)
    idx = capi.Index(gpu_ctx, genomic)
    ops = SL.OracleOps(genomic)
    originals = {k: with_a_polyA_tail(seqs[k]) for k in range(0, n_pat, 3)}
    originals = {k: o for k, o in originals.items() if o != seqs[k]}
    assert len(originals) > 80
    try:
        for resident in (False, True):
            plain = capi.PairingPlan(gpu_ctx, idx, seqs, resident=resident)
            try:
                want_plain = run_plan(plain, prm)
                cres, cex = plain.fetch_candidates()
            finally:
                plain.close()
            plan = capi.PairingPlan(gpu_ctx, idx, seqs, resident=resident, originals=originals)
            try:
                got = run_plan(plan, prm)
                assert plan.fetch_candidates()[0].tobytes() == cres.tobytes()              # the originals take no part before
                mine, differ = [], 0
                for k in range(n_pat):
                    lo, n = int(cres["first_exon"][k]), int(cres["n_exons"][k])
                    ex = [tuple(int(v) for v in e) for e in cex[lo:lo + n]]
                    mine.append(FL.final(int(cres["kind"][k]), originals.get(k, seqs[k]), seqs[k], genomic, ex, ops=ops))
                same(got, FL.expect_arrays(mine), "originals")
                for k in range(n_pat):
                    a, b = sub_results(got, [k]), sub_results(want_plain, [k])
                    equal = all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
                    if k not in originals:
                        assert equal, k
                    differ += not equal
                assert differ >= 10, differ
                # the index form with the same originals behind the patterns
                off = np.zeros(n_pat + 1, dtype=np.uint64)
                np.cumsum([len(s) for s in seqs], out=off[1:])
                orig_off = off[:-1].copy()
                blob, at = b"".join(seqs), int(off[-1])
                for k in sorted(originals):
                    orig_off[k] = at
                    at += len(originals[k])
                blob += b"".join(originals[k] for k in sorted(originals))
                q = FL.plan_queries(off, cres, orig_off)
                r2, e2, s2 = device(idx, blob, cex, q, F.DEFAULTS, 40)
                same(got, (FL.stage0_of_kinds(r2, cres["kind"]), e2, s2), "originals, index form")
            finally:
                plan.close()
    finally:
        idx.close()


def test_the_rules_of_the_fifth_rung_and_the_refusals(gpu_ctx):
    import pintron_amd.capi as capi
    L_ = gpu_ctx.L
    gfa, efa = M.rerun_input()
    exp, genomic = M.first_attempt_megs(gfa, efa)
    seqs = [e["seq"] for e in exp]
    seqs = seqs[:10] + [b""] + seqs[10:]                                                    # an empty pattern is legal
    idx = capi.Index(gpu_ctx, genomic)
    plan = capi.PairingPlan(gpu_ctx, idx, seqs)

    def message():
        return L_.pgpu_last_error(gpu_ctx.h).decode()

    def fetch_refused():
        return plan.fetch_final_factorizations_raw(4096)[0] == capi.PGPU_EINVAL and "run_final_factorizations first" in message()
    try:
        assert fetch_refused()                                                              # nothing ran yet
        assert plan.run_final_factorizations_raw() == capi.PGPU_EINVAL and "run_factorizations" in message()
        plan.run(15, 0.2)
        plan.run_meg(**M.DEFAULTS)
        plan.run_candidates(15, 40)
        assert plan.run_final_factorizations_raw() == capi.PGPU_EINVAL and "run_factorizations" in message()
        plan.run_factorizations(*F.DEFAULTS)
        fact = plan.fetch_factorizations()
        assert fetch_refused()
        assert plan.run_final_factorizations_raw(no_params=True) == capi.PGPU_EINVAL
        assert plan.run_final_factorizations_raw(reserved=1) == capi.PGPU_EINVAL and message() == BAD_SMALL
        assert fetch_refused() and L_.pgpu_pairing_plan_final_exons(plan.h) == 0 and plan.final_ms(0) == 0.0
        n = plan.run_final_factorizations(40)
        assert n > 0 and plan.final_ms(0) > 0.0 and plan.final_ms(3) == 0.0 and plan.final_ms(-1) == 0.0
        assert L_.pgpu_pairing_plan_final_exons(None) == 0 and L_.pgpu_pairing_plan_final_ms(None, 0) == 0.0
        want = plan.fetch_final_factorizations()
        assert int(want[0]["n_exons"].sum()) == n
        empty = tuple(int(v) for v in want[0][10])                                                 # the empty pattern: no candidate
        assert empty[:2] == (FL.HOST, 0) and empty[2] in (KL.NONE, KL.NOT_PATH) and not any(empty[3:]), empty
        without = capi.PairingPlan(gpu_ctx, idx, seqs[:10] + seqs[11:])
        try:
            others = list(range(10)) + list(range(11, len(seqs)))
            same(sub_results(want, others), run_plan(without, M.DEFAULTS), "beside an empty pattern")
        finally:
            without.close()
        assert plan.fetch_final_factorizations_raw(n - 1)[0] == capi.PGPU_ENOSPC and message() == "exon buffer too small"
        assert all(a.tobytes() == b.tobytes() for a, b in zip(plan.fetch_factorizations(), fact))      # unchanged and fetchable
        assert plan.run_final_factorizations(-7) >= 0 and plan.run_final_factorizations(40) == n     # any min_intron_length
        assert all(a.tobytes() == b.tobytes() for a, b in zip(plan.fetch_final_factorizations(), want))
        # a run of any earlier stage takes the finals with it
        for rerun in (lambda: plan.run_factorizations(*F.DEFAULTS), lambda: plan.run_candidates(15, 40),
                      lambda: plan.run_meg(**M.DEFAULTS), lambda: plan.run(15, 0.2)):
            rerun()
            assert fetch_refused()
            plan.run(15, 0.2)
            plan.run_meg(**M.DEFAULTS)
            plan.run_candidates(15, 40)
            plan.run_factorizations(*F.DEFAULTS)
            assert plan.run_final_factorizations(40) == n
            assert all(a.tobytes() == b.tobytes() for a, b in zip(plan.fetch_final_factorizations(), want))
    finally:
        plan.close()
    # an empty plan
    for resident in (False, True):
        empty = capi.PairingPlan(gpu_ctx, idx, [], resident=resident)
        try:
            assert empty.run_candidates(15, 40) == 0 and empty.run_factorizations(*F.DEFAULTS) == 0
            assert empty.run_final_factorizations(40) == 0 and empty.final_ms(0) == 0.0
            assert L_.pgpu_pairing_plan_fetch_final_factorizations(gpu_ctx.h, empty.h, None, None, None, 0) == capi.PGPU_OK
        finally:
            empty.close()
    # every refusal of create_with_originals
    blob = b"".join(seqs)
    off = np.zeros(len(seqs) + 1, dtype=np.uint64)
    np.cumsum([len(s) for s in seqs], out=off[1:])

    def create(pats, origs, null_lists=False, resident=False):
        h = C.c_void_p()
        rc = capi.PairingPlan.create_with_originals_raw(gpu_ctx, idx, blob, off, len(seqs), resident, np.array(pats, dtype=np.uint32), origs,
                                                        h, null_lists)
        if rc == capi.PGPU_OK:
            L_.pgpu_pairing_plan_destroy(gpu_ctx.h, h)
        else:
            assert not h.value
        return rc
    for resident in (False, True):
        assert create([0, 2], [seqs[0], seqs[2]], resident=resident) == capi.PGPU_OK
        assert create([], [], null_lists=True, resident=resident) == capi.PGPU_OK
        assert create([len(seqs)], [seqs[0]], resident=resident) == capi.PGPU_EINVAL and "beyond" in message()
        assert create([2, 0], [seqs[2], seqs[0]], resident=resident) == capi.PGPU_EINVAL and "ascending" in message()
        assert create([2, 2], [seqs[2], seqs[2]], resident=resident) == capi.PGPU_EINVAL and "ascending" in message()
        assert create([0], [seqs[0][:-1]], resident=resident) == capi.PGPU_EINVAL and "length" in message()
        assert create([0], [seqs[0] + b"A"], resident=resident) == capi.PGPU_EINVAL and "length" in message()
        assert create([0], [seqs[0]], null_lists=True, resident=resident) == capi.PGPU_EINVAL and "null" in message()
    idx.close()
