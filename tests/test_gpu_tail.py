"""GPU: pgpu_index_tail_chains against the fixture that the reference's object code, the restatement and the host's
ef_chain_tail agreed on (the golden cases), against today's route on the device (DP plans of PGPU_DP_AFFIX, PGPU_DP_ED and
PGPU_DP_BORDERS jobs with the host logic of tests/tail_lib.py around them), and against the restatement (tests/tail_lib.py)
-- never against the library under test alone.  Every comparison is byte equality."""
import ctypes as C

import numpy as np
import pytest

import tail_lib as TL

pytestmark = pytest.mark.gpu

MESSAGE = ("bad tail query (a range past its buffer, an empty EST, reserved != 0, no exon, an exon two queries share, or a "
           "coordinate that is no byte of what it indexes)")


@pytest.fixture(scope="module")
def golden(gpu_ctx):
    import pintron_amd.capi as capi
    gen, hand, real = TL.load_fixture()
    idx = capi.Index(gpu_ctx, gen)
    yield gen, hand, idx
    idx.close()


def golden_answers(cases):
    return [c["answer"] for c in cases]


def check(idx, ests, exons, q, want_arrays):
    out_exons, out_steps, res = idx.tail_chains(ests, exons, q)
    we, ws, wr = want_arrays
    for name, got, want in (("results", res, wr), ("steps", out_steps, ws), ("exons", out_exons, we)):
        if got.tobytes() != want.tobytes():
            bad = [i for i in range(len(got)) if got[i] != want[i]]
            raise AssertionError("%s differ at %d places, first %d: %r / %r" % (name, len(bad), bad[0], got[bad[0]], want[bad[0]]))
    return out_exons, out_steps, res


def test_every_golden_case_in_one_call_and_again(golden):
    gen, cases, idx = golden
    ests, exons, q = TL.batch_arrays(TL.quads(cases))
    first = check(idx, ests, exons, q, TL.expect_arrays(exons, golden_answers(cases)))
    assert idx.tail_chains_kernel_ms() > 0.0                   # the fixture's context has timing on
    again = idx.tail_chains(ests, exons, q)                    # the same call twice on one context gives the same bytes
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, again))


def test_golden_cases_on_a_loaded_index(golden, gpu_ctx, tmp_path):
    import pintron_amd.capi as capi
    gen, cases, idx = golden
    ests, exons, q = TL.batch_arrays(TL.quads(cases))
    path = str(tmp_path / "tail.idx")
    idx.save(path)
    loaded = capi.Index(gpu_ctx, gen, load_from=path)
    try:
        check(loaded, ests, exons, q, TL.expect_arrays(exons, golden_answers(cases)))
    finally:
        loaded.close()


@pytest.mark.parametrize("source", ["c2", "ambn", "issue13"])
def test_golden_cases_of_the_real_inputs(source, gpu_ctx):
    import cand_lib as KL
    import meg_lib as M
    import pintron_amd.capi as capi
    cases = TL.load_fixture()[2][source]
    genomic = M.first_attempt_megs(*KL.real_inputs()[source][:2], M.DEFAULTS)[1]
    ests, exons, q = TL.batch_arrays(TL.quads(cases))
    idx = capi.Index(gpu_ctx, genomic)
    try:
        check(idx, ests, exons, q, TL.expect_arrays(exons, golden_answers(cases)))
    finally:
        idx.close()


def test_two_thousand_fresh_queries_against_the_restatement_and_todays_route(golden, gpu_ctx):
    gen, _, idx = golden
    batch = TL.generated(2026, gen, 2000)
    infos = [{} for _ in batch]
    want = [TL.tail(orig, est, gen, ex, info=i) for (_, orig, est, ex), i in zip(batch, infos)]
    assert all(w[0] == TL.OK for w in want)
    assert sum(i.get("dp_affix", 0) for i in infos) > 200 and sum(i.get("dp_borders", 0) for i in infos) > 2000
    assert sum(w[4] != 0 for w in want) > 50 and sum(w[2] for w in want) > 50 and sum(w[6] > 0 for w in want) > 200
    ests, exons, q = TL.batch_arrays(batch)
    check(idx, ests, exons, q, TL.expect_arrays(exons, want))
    clock = {}
    assert TL.device_route(gpu_ctx, idx, gen, batch, clock=clock) == want
    assert clock["jobs"] > 2000 and clock["rounds"] >= 2


def test_every_cap_edge_in_one_batch_between_neighbours(golden):
    gen, cases, idx = golden
    edges = ["exons_64", "exons_65", "affix_64", "affix_65", "affix_256", "affix_257", "exon_100", "exon_101", "window_128", "window_129",
             "gen_256", "gen_257", "ext_63", "ext_64", "ext_65", "front_suffix", "removed_twice"]
    picked = [next(c for c in cases if t in c["tags"]) for t in edges]
    picked += [next(c for c in cases if c["name"] == n) for n in ("pre_w257_skipped", "suf_w257_skipped", "pre_w257", "suf_w257")]
    ordinary = [c for c in cases if c["answer"][:2] == (TL.OK, 0) and len(c["exons"]) >= 2 and any(s & 3 for s in c["answer"][8])][:3]
    batch = []
    for k, c in enumerate(picked):
        batch += [ordinary[k % 3], c]
    batch.append(ordinary[0])
    ests, exons, q = TL.batch_arrays(TL.quads(batch))
    we, ws, wr = TL.expect_arrays(exons, golden_answers(batch))
    refused = wr["status"] == TL.ERANGE
    assert refused.sum() == 6
    for i in np.flatnonzero(refused):                          # a refused query leaves its exons untouched, and everything else 0
        lo, n = int(q[i]["first_exon"]), int(q[i]["n_exons"])
        assert we[lo:lo + n].tobytes() == exons[lo:lo + n].tobytes() and not ws[lo:lo + n].any()
        assert bytes(wr[i].tobytes()[4:]) == bytes(12)
    check(idx, ests, exons, q, (we, ws, wr))
    # each picked case alone comes out as it does between its neighbours
    for c in picked[:6]:
        e1, x1, q1 = TL.batch_arrays(TL.quads([c]))
        check(idx, e1, x1, q1, TL.expect_arrays(x1, golden_answers([c])))
    # exons that no query names, in front and behind: copied, with step 0
    loose = np.array([(7, 9, 11, 13), (-1, -1, -1, -1)], dtype=exons.dtype)
    q_l = q.copy()
    q_l["first_exon"] += 1
    check(idx, ests, np.concatenate([loose[:1], exons, loose[1:]]), q_l,
          (np.concatenate([loose[:1], we, loose[1:]]), np.concatenate([[0], ws, [0]]).astype(np.uint8), wr))


def test_a_query_that_asks_nothing_is_answered(golden):
    """no affix DP (equal first bytes, or nothing in front of / behind the factorization) and no analysis (one or two exons,
    or an inner exon of more than 100 bytes): the restatement counts no question, and the entry answers all the same"""
    gen, cases, idx = golden
    quiet = []
    for c in cases:
        info = {}
        a = TL.tail(c["orig"], c["est"], gen, c["exons"], info=info)
        if a[0] == TL.OK and not (info.get("dp_affix") or info.get("dp_ed") or info.get("dp_borders")):
            quiet.append(c)
    names = {c["name"] for c in quiet}
    assert len(quiet) > 100 and {"pre_skipped", "suf_skipped", "pre_w257_skipped", "small_e101", "inv_est_pair"} <= names, sorted(names)
    ests, exons, q = TL.batch_arrays(TL.quads(quiet))
    check(idx, ests, exons, q, TL.expect_arrays(exons, golden_answers(quiet)))


def test_refusals_and_the_contract_of_the_entry(golden, gpu_ctx):
    import pintron_amd.capi as capi
    L = capi.lib()
    gen, cases, idx = golden
    glen = len(gen)
    some = [c for c in cases if c["answer"][:2] == (TL.OK, 0) and len(c["exons"]) >= 3 and any(s & 3 for s in c["answer"][8])][:5]
    some.append(next(c for c in cases if "orig_differs" in c["tags"]))
    ests, exons, q = TL.batch_arrays(TL.quads(some))
    want = TL.expect_arrays(exons, golden_answers(some))
    n_ex = len(exons)
    f = L.pgpu_index_tail_chains

    def raw(ests_, e_, q_, n):
        """the call with its three outputs filled beforehand -> (rc, whether anything was written)"""
        oe = np.full(len(e_), 0x55, dtype=np.uint8).repeat(16).view(np.dtype(capi.FACTOR_DTYPE))
        ob = np.full(len(e_), 0x55, dtype=np.uint8)
        orr = np.full(16 * max(n, 1), 0x55, dtype=np.uint8).view(np.dtype(capi.TAIL_RESULT_DTYPE))
        rc = f(gpu_ctx.h, idx.h, ests_, len(ests_), e_.ctypes.data_as(C.POINTER(capi.Factor)), len(e_),
               q_.ctypes.data_as(C.POINTER(capi.TailQuery)), n, oe.ctypes.data_as(C.POINTER(capi.Factor)),
               ob.ctypes.data_as(C.POINTER(C.c_uint8)), orr.ctypes.data_as(C.POINTER(capi.TailResult)))
        untouched = all((x.view(np.uint8) == 0x55).all() for x in (oe, ob, orr))
        return rc, untouched

    def rc_of(mod_q=None, mod_e=None, ests_=None):
        q2, e2 = q.copy(), exons.copy()
        if mod_q:
            mod_q(q2)
        if mod_e:
            mod_e(e2)
        b = ests if ests_ is None else ests_
        rc, untouched = raw(b, e2, q2, len(q2))
        assert (rc == capi.PGPU_EINVAL) == TL.einval(len(b), glen, e2, q2) and rc in (capi.PGPU_OK, capi.PGPU_EINVAL)
        if rc == capi.PGPU_EINVAL:
            assert L.pgpu_last_error(gpu_ctx.h).decode() == MESSAGE and idx.tail_chains_kernel_ms() == 0.0 and untouched
        return rc

    def put(field, i, value):
        def mod(x):
            x[field][i] = value
        return mod
    f1 = int(q[1]["first_exon"])
    el1 = int(q[1]["est_len"])
    bad_q = [put("n_exons", 2, 0), put("n_exons", len(q) - 1, int(q[-1]["n_exons"]) + 1), put("first_exon", 3, len(exons)),
             put("first_exon", 3, 0xFFFFFFFF), put("est_off", 1, len(ests)), put("est_off", 1, 1 << 40), put("est_len", 1, 0xFFFFFFFF),
             put("est_len", 1, 0x80000000), put("est_len", 1, 0), put("reserved", 4, 1), put("first_exon", 1, f1 - 1),
             put("n_exons", 0, int(q[0]["n_exons"]) + 1), put("orig_off", 1, len(ests) - el1 + 1), put("orig_off", 1, 1 << 40),
             put("orig_off", 1, 0xFFFFFFFFFFFFFFFF)]
    for k, mod in enumerate(bad_q):
        check(idx, ests, exons, q, want)                                          # a slot for the refusal to reset
        assert idx.tail_chains_kernel_ms() > 0.0
        assert rc_of(mod_q=mod) == capi.PGPU_EINVAL, k
    assert rc_of(mod_q=put("orig_off", 1, len(ests) - el1)) == capi.PGPU_OK       # the last place the original fits
    bad_e = [put("EST_start", f1 + 1, -1), put("EST_end", f1 + 1, el1), put("GEN_start", f1 + 1, -1), put("GEN_end", f1 + 1, glen),
             put("EST_start", f1, el1), put("EST_end", f1, -1), put("GEN_start", f1, glen), put("GEN_end", f1, -1)]
    for k, mod in enumerate(bad_e):
        assert rc_of(mod_e=mod) == capi.PGPU_EINVAL, k
    for mod in (put("EST_end", f1 + 1, el1 - 1), put("GEN_end", f1 + 1, glen - 1), put("EST_start", f1 + 1, 0), put("GEN_start", f1 + 1, 0),
                put("EST_end", f1, int(exons[f1 + 1]["EST_start"]))):                # out of order: step 3's verdict, no refusal
        assert rc_of(mod_e=mod) == capi.PGPU_OK
    assert rc_of(ests_=ests[:-1]) == capi.PGPU_EINVAL                             # the last sequence runs past the buffer
    # the refusal is repeated after a good call
    for _ in range(2):
        check(idx, ests, exons, q, want)
        assert idx.tail_chains_kernel_ms() > 0.0
        assert rc_of(mod_q=put("reserved", 0, 1)) == capi.PGPU_EINVAL
    # null pointers: a bare refusal, the message stays; n == 0
    oe, ob = np.zeros_like(exons), np.full(n_ex, 9, dtype=np.uint8)
    orr = np.zeros(len(q), dtype=np.dtype(capi.TAIL_RESULT_DTYPE))
    ep, qp = exons.ctypes.data_as(C.POINTER(capi.Factor)), q.ctypes.data_as(C.POINTER(capi.TailQuery))
    oep, obp, orp = oe.ctypes.data_as(C.POINTER(capi.Factor)), ob.ctypes.data_as(C.POINTER(C.c_uint8)), orr.ctypes.data_as(C.POINTER(capi.TailResult))
    check(idx, ests, exons, q, want)
    for args in ((None, ests, ep, qp, oep, obp, orp), (idx.h, None, ep, qp, oep, obp, orp), (idx.h, ests, None, qp, oep, obp, orp),
                 (idx.h, ests, ep, None, oep, obp, orp), (idx.h, ests, ep, qp, None, obp, orp), (idx.h, ests, ep, qp, oep, None, orp),
                 (idx.h, ests, ep, qp, oep, obp, None)):
        ih, es, e_, q_, oe_, ob_, or_ = args
        assert f(gpu_ctx.h, ih, es, len(ests), e_, n_ex, q_, len(q), oe_, ob_, or_) == capi.PGPU_EINVAL
        assert L.pgpu_last_error(gpu_ctx.h).decode() == MESSAGE                   # of the refusal before: untouched
        assert idx.tail_chains_kernel_ms() == 0.0
    assert f(None, idx.h, ests, len(ests), ep, n_ex, qp, len(q), oep, obp, orp) == capi.PGPU_EINVAL
    check(idx, ests, exons, q, want)
    assert idx.tail_chains_kernel_ms() > 0.0
    assert f(gpu_ctx.h, idx.h, ests, len(ests), ep, n_ex, None, 0, oep, obp, None) == capi.PGPU_OK       # n == 0: a copy
    assert oe.tobytes() == exons.tobytes() and not ob.any() and idx.tail_chains_kernel_ms() == 0.0
    assert f(gpu_ctx.h, idx.h, None, 0, None, 0, None, 0, None, None, None) == capi.PGPU_OK
    check(idx, ests, exons, q, want)                                              # the context still answers


def test_without_timing_the_answers_are_the_same(golden):
    import pintron_amd.capi as capi
    gen, cases, _ = golden
    ests, exons, q = TL.batch_arrays(TL.quads(cases[:120]))
    want = TL.expect_arrays(exons, golden_answers(cases[:120]))
    with capi.Context(0) as ctx:
        idx = capi.Index(ctx, gen)
        check(idx, ests, exons, q, want)
        assert idx.tail_chains_kernel_ms() > 0.0
        ctx.L.pgpu_set_timing(ctx.h, 0)
        check(idx, ests, exons, q, want)
        assert idx.tail_chains_kernel_ms() == 0.0
        idx.close()
