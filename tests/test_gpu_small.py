"""GPU: pgpu_index_small_chains against the fixture that the reference's refine_EST_factorizations, the restatement and the
host's ef_chain_small agreed on (the golden cases), against today's route on the device (DP plans of PGPU_DP_LCF,
PGPU_DP_ED, PGPU_DP_BORDERS and PGPU_DP_KBAND jobs, pgpu_index_classify and pgpu_index_small_exons, with the host logic of
tests/small_lib.py around them), and against the restatement (tests/small_lib.py) -- never against the library under test
alone.  Every comparison is byte equality.  min_intron_length is a parameter of the call, so a batch is one call per value."""
import ctypes as C

import numpy as np
import pytest

import small_lib as SL

pytestmark = pytest.mark.gpu

MESSAGE = ("bad small query (a range past its buffer, an empty EST, reserved != 0, no exon, an exon two queries share, or a "
           "coordinate that is no byte of what it indexes)")
PARAMS_MESSAGE = "bad small-chains parameters (reserved != 0)"


@pytest.fixture(scope="module")
def golden(gpu_ctx):
    """the fixture's first sequence (every builder's cases but the one-locus ones) with its index"""
    import pintron_amd.capi as capi
    worlds, _ = SL.load_fixture()
    gen, hand = worlds[0]
    idx = capi.Index(gpu_ctx, gen)
    yield gen, hand, idx
    idx.close()


def answers(cases):
    return [c["answer"] for c in cases]


def check(idx, ests, exons, q, mil, want_arrays):
    out_exons, out_steps, res = idx.small_chains(ests, exons, q, mil)
    we, ws, wr = want_arrays
    assert len(out_exons) == len(out_steps) == 2 * len(exons)
    for name, got, want in (("results", res, wr), ("steps", out_steps, ws), ("exons", out_exons, we)):
        if got.tobytes() != want.tobytes():
            bad = [i for i in range(len(got)) if got[i] != want[i]]
            raise AssertionError("%s differ at %d places, first %d: %r / %r" % (name, len(bad), bad[0], got[bad[0]], want[bad[0]]))
    return out_exons, out_steps, res


def by_mil(cases):
    """the cases (dicts of the fixture) in one group per min_intron_length, in their order"""
    groups = {}
    for c in cases:
        groups.setdefault(c["mil"], []).append(c)
    return sorted(groups.items())


def check_cases(idx, cases):
    """one call per min_intron_length -> the outputs of every call"""
    out = []
    for mil, group in by_mil(cases):
        ests, exons, q = SL.batch_arrays(SL.quints(group))
        out.append(check(idx, ests, exons, q, mil, SL.expect_arrays(exons, q, answers(group))))
    return out


def test_every_golden_case_in_one_call_per_parameter_and_again(golden):
    gen, cases, idx = golden
    first = check_cases(idx, cases)
    assert idx.small_chains_kernel_ms() > 0.0                  # the fixture's context has timing on
    again = check_cases(idx, cases)                            # the same calls twice on one context give the same bytes
    assert all(a.tobytes() == b.tobytes() for x, y in zip(first, again) for a, b in zip(x, y))


def test_golden_cases_on_a_loaded_index(golden, gpu_ctx, tmp_path):
    import pintron_amd.capi as capi
    gen, cases, idx = golden
    path = str(tmp_path / "small.idx")
    idx.save(path)
    loaded = capi.Index(gpu_ctx, gen, load_from=path)
    try:
        check_cases(loaded, cases)                             # the classification tables are built on first use here too
    finally:
        loaded.close()


def test_golden_cases_of_the_one_locus_sequences(gpu_ctx):
    """what depends on the whole sequence in front of the first exon: the first byte that is no upper-case ACGT at the exon's
    start and one byte earlier, splice sites in mixed and lower case in front of the exon (refused) and at its start (a
    lower-case gt .. ag accepted, a mixed-case one not), common factors of five and six bytes.  Each case stands in one
    batch between two ordinary neighbours of its sequence, and comes out alone as it does there."""
    import pintron_amd.capi as capi
    worlds, _ = SL.load_fixture()
    seen, accepted_lower = set(), 0
    for gen, cases in worlds[1:]:
        assert [c["name"] for c in cases][::2] == ["beside_between", "beside_plain"] and len({c["mil"] for c in cases}) == 1
        assert cases[0]["answer"][0] == cases[2]["answer"][0] == SL.OK and cases[0]["answer"][4] == 1
        idx = capi.Index(gpu_ctx, gen)
        try:
            (_, _, res), = check_cases(idx, cases)
            check_cases(idx, cases[1:2])
        finally:
            idx.close()
        seen.add(cases[1]["name"])
        if "lower_gtag" in cases[1]["tags"]:
            assert res[1]["status"] == SL.OK and res[1]["prefix_added"] == 1
            accepted_lower += 1
    assert seen == set(SL.MINI_KINDS) and accepted_lower >= SL.MIN_PER_TAG


@pytest.mark.parametrize("source", ["c2", "ambn", "issue13"])
def test_golden_cases_of_the_real_inputs(source, gpu_ctx):
    import cand_lib as KL
    import meg_lib as M
    import pintron_amd.capi as capi
    cases = SL.load_fixture()[1][source]
    genomic = M.first_attempt_megs(*KL.real_inputs()[source][:2], M.DEFAULTS)[1]
    idx = capi.Index(gpu_ctx, genomic)
    try:
        check_cases(idx, cases)
    finally:
        idx.close()


def test_two_thousand_fresh_queries_against_the_restatement_and_todays_route(gpu_ctx):
    import pintron_amd.capi as capi
    gen, batch = SL.generated(2026, 2000)
    ops = SL.OracleOps(gen)
    infos = [{} for _ in batch]
    want = [SL.small(o, e, gen, ex, mil, ops=ops, info=i) for (_, o, e, ex, mil), i in zip(batch, infos)]
    assert all(w[0] == SL.OK for w in want)
    assert sum(w[3] for w in want) >= 200 and sum(w[4] - w[3] > 0 for w in want) >= 200 and sum(w[7] < w[5] for w in want) >= 200
    assert sum(i.get("dp_borders", 0) for i in infos) > 200 and sum(i.get("dp_sexon", 0) for i in infos) > 400
    idx = capi.Index(gpu_ctx, gen)
    try:
        for mil in sorted({c[4] for c in batch}):
            group = [(c, w) for c, w in zip(batch, want) if c[4] == mil]
            ests, exons, q = SL.batch_arrays([c for c, _ in group])
            check(idx, ests, exons, q, mil, SL.expect_arrays(exons, q, [w for _, w in group]))
        clock = {}
        assert SL.device_route(gpu_ctx, idx, gen, batch, clock=clock) == want
        assert clock["jobs"] > 2000 and clock["rounds"] >= 3
    finally:
        idx.close()


def test_every_cap_edge_in_one_batch_between_neighbours(golden):
    gen, cases, idx = golden
    at_60 = [c for c in cases if c["mil"] == 60]
    edges = ["grow_past_64", "exons_65", "window_256", "window_257", "piece_one_n", "piece_two_n", "kband_31", "kband_32", "disordered",
             "est_start_6", "est_start_7", "est_start_46", "est_start_47", "pair_gate_51", "pair_gate_52", "gate_28", "gate_29",
             "three_insertions", "inserted_dropped", "emptied_noisy", "emptied_external", "offp_wraps"]
    picked = [next(c for c in at_60 if t in c["tags"]) for t in edges]
    picked.append(next(c for c in at_60 if c["name"] == "piece_lower"))
    ordinary = [next(c for c in at_60 if c["name"] == n) for n in ("prefix_found", "between_found_k0", "dist_0")]
    batch = []
    for k, c in enumerate(picked):
        batch += [ordinary[k % 3], c]
    batch.append(ordinary[0])
    ests, exons, q = SL.batch_arrays(SL.quints(batch))
    we, ws, wr = SL.expect_arrays(exons, q, answers(batch))
    refused = wr["status"] == SL.ERANGE
    assert sorted(wr["refused"][refused].tolist()) == [1, 2, 3, 3, 4, 5]
    for i in np.flatnonzero(refused):          # a refused query leaves its exons at its place in the output, and everything else 0
        lo, n = int(q[i]["first_exon"]), int(q[i]["n_exons"])
        assert we[2 * lo:2 * lo + n].tobytes() == exons[lo:lo + n].tobytes() and not we[2 * lo + n:2 * lo + 2 * n].tobytes().strip(b"\0")
        assert not ws[2 * lo:2 * lo + 2 * n].any()
        assert bytes(wr[i].tobytes()[5:]) == bytes(19) and wr[i]["refused"] in (1, 2, 3, 4, 5)
    check(idx, ests, exons, q, 60, (we, ws, wr))
    # each picked case alone comes out as it does between its neighbours
    for c in picked:
        check_cases(idx, [c])
    # exons that no query names, in front and behind: their two slots are 0
    loose = np.array([(7, 9, 11, 13), (-1, -1, -1, -1)], dtype=exons.dtype)
    q_l = q.copy()
    q_l["first_exon"] += 1
    zero2 = np.zeros(2, dtype=exons.dtype)
    check(idx, ests, np.concatenate([loose[:1], exons, loose[1:]]), q_l, 60,
          (np.concatenate([zero2, we, zero2]), np.concatenate([[0, 0], ws, [0, 0]]).astype(np.uint8), wr))


def test_a_query_that_asks_nothing_is_answered(golden):
    """no common factor, no edit distance, no refinement, no search (one exon at the EST's first bytes, two short exons): the
    restatement counts none of those questions, and the entry answers all the same"""
    gen, cases, idx = golden
    ops = SL.OracleOps(gen)
    quiet = []
    for c in cases:
        info = {}
        a = SL.small(c["orig"], c["est"], gen, c["exons"], c["mil"], ops=ops, info=info)
        if a[0] == SL.OK and not any(info.get(k) for k in ("dp_lcf", "dp_ed", "dp_borders", "dp_lcf_small", "dp_sexon")):
            quiet.append(c)
    names = {c["name"] for c in quiet}
    assert len(quiet) >= 10 and {"est_start_6", "gate_28", "pair_gate_51", "dist_0", "emptied_external"} <= names, sorted(names)
    check_cases(idx, quiet)


def test_refusals_and_the_contract_of_the_entry(golden, gpu_ctx):
    import pintron_amd.capi as capi
    L = capi.lib()
    gen, cases, idx = golden
    glen = len(gen)
    at_60 = [c for c in cases if c["mil"] == 60 and c["answer"][0] == SL.OK]
    some = [c for c in at_60 if len(c["exons"]) >= 2 and c["answer"][4] > 0][:5]
    some.append(next(c for c in at_60 if "orig_decides" in c["tags"]))
    ests, exons, q = SL.batch_arrays(SL.quints(some))
    want = SL.expect_arrays(exons, q, answers(some))
    n_ex = len(exons)
    f = L.pgpu_index_small_chains
    good = capi.SmallParams(60, 0)

    def raw(ests_, e_, q_, n, prm):
        """the call with its three outputs filled beforehand -> (rc, whether anything was written)"""
        oe = np.full(2 * len(e_), 0x55, dtype=np.uint8).repeat(16).view(np.dtype(capi.FACTOR_DTYPE))
        ob = np.full(2 * len(e_), 0x55, dtype=np.uint8)
        orr = np.full(24 * max(n, 1), 0x55, dtype=np.uint8).view(np.dtype(capi.SMALL_RESULT_DTYPE))
        rc = f(gpu_ctx.h, idx.h, ests_, len(ests_), e_.ctypes.data_as(C.POINTER(capi.Factor)), len(e_),
               q_.ctypes.data_as(C.POINTER(capi.SmallQuery)), n, prm, oe.ctypes.data_as(C.POINTER(capi.Factor)),
               ob.ctypes.data_as(C.POINTER(C.c_uint8)), orr.ctypes.data_as(C.POINTER(capi.SmallResult)))
        untouched = all((x.view(np.uint8) == 0x55).all() for x in (oe, ob, orr))
        return rc, untouched

    def rc_of(mod_q=None, mod_e=None, ests_=None):
        q2, e2 = q.copy(), exons.copy()
        if mod_q:
            mod_q(q2)
        if mod_e:
            mod_e(e2)
        b = ests if ests_ is None else ests_
        rc, untouched = raw(b, e2, q2, len(q2), C.byref(good))
        assert (rc == capi.PGPU_EINVAL) == SL.einval(len(b), glen, e2, q2) and rc in (capi.PGPU_OK, capi.PGPU_EINVAL)
        if rc == capi.PGPU_EINVAL:
            assert L.pgpu_last_error(gpu_ctx.h).decode() == MESSAGE and idx.small_chains_kernel_ms() == 0.0 and untouched
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
        check(idx, ests, exons, q, 60, want)                                      # a slot for the refusal to reset
        assert idx.small_chains_kernel_ms() > 0.0
        assert rc_of(mod_q=mod) == capi.PGPU_EINVAL, k
    assert rc_of(mod_q=put("orig_off", 1, len(ests) - el1)) == capi.PGPU_OK       # the last place the original fits
    bad_e = [put("EST_start", f1 + 1, -1), put("EST_end", f1 + 1, el1), put("GEN_start", f1 + 1, -1), put("GEN_end", f1 + 1, glen),
             put("EST_start", f1, el1), put("EST_end", f1, -1), put("GEN_start", f1, glen), put("GEN_end", f1, -1)]
    for k, mod in enumerate(bad_e):
        assert rc_of(mod_e=mod) == capi.PGPU_EINVAL, k
    for mod in (put("EST_end", f1 + 1, el1 - 1), put("GEN_end", f1 + 1, glen - 1),
                put("EST_end", f1, int(exons[f1 + 1]["EST_start"]))):                # out of order: refused = 5 on the device, good input
        assert rc_of(mod_e=mod) == capi.PGPU_OK
    assert rc_of(ests_=ests[:-1]) == capi.PGPU_EINVAL                             # the last sequence runs past the buffer
    # the parameters: reserved != 0 with its own message, a null pointer bare
    check(idx, ests, exons, q, 60, want)
    rc, untouched = raw(ests, exons, q, len(q), C.byref(capi.SmallParams(60, 1)))
    assert rc == capi.PGPU_EINVAL and untouched and L.pgpu_last_error(gpu_ctx.h).decode() == PARAMS_MESSAGE
    assert idx.small_chains_kernel_ms() == 0.0
    rc, untouched = raw(ests, exons, q, len(q), None)
    assert rc == capi.PGPU_EINVAL and untouched and L.pgpu_last_error(gpu_ctx.h).decode() == PARAMS_MESSAGE
    rc, untouched = raw(ests, exons, q, 0, C.byref(capi.SmallParams(60, 1)))      # an empty call is refused the same way: nothing written
    assert rc == capi.PGPU_EINVAL and untouched and L.pgpu_last_error(gpu_ctx.h).decode() == PARAMS_MESSAGE
    # any min_intron_length is a good parameter: the extremes are answered as the restatement answers them
    ops = SL.OracleOps(gen)
    for mil in (-2147483648, -1, 0, 4, 2147483647):
        w = [SL.small(c["orig"], c["est"], gen, c["exons"], mil, ops=ops) for c in some]
        check(idx, ests, exons, q, mil, SL.expect_arrays(exons, q, w))
    # the refusal is repeated after a good call
    for _ in range(2):
        check(idx, ests, exons, q, 60, want)
        assert idx.small_chains_kernel_ms() > 0.0
        assert rc_of(mod_q=put("reserved", 0, 1)) == capi.PGPU_EINVAL
    # null pointers: a bare refusal, the message stays; n == 0
    oe, ob = np.full(2 * n_ex, 9, dtype=np.uint8).repeat(16).view(exons.dtype), np.full(2 * n_ex, 9, dtype=np.uint8)
    orr = np.zeros(len(q), dtype=np.dtype(capi.SMALL_RESULT_DTYPE))
    ep, qp = exons.ctypes.data_as(C.POINTER(capi.Factor)), q.ctypes.data_as(C.POINTER(capi.SmallQuery))
    oep, obp, orp = oe.ctypes.data_as(C.POINTER(capi.Factor)), ob.ctypes.data_as(C.POINTER(C.c_uint8)), orr.ctypes.data_as(C.POINTER(capi.SmallResult))
    pp = C.byref(good)
    check(idx, ests, exons, q, 60, want)
    assert rc_of(mod_q=put("reserved", 0, 1)) == capi.PGPU_EINVAL                 # (the message the bare refusals leave alone)
    for args in ((None, ests, ep, qp, oep, obp, orp), (idx.h, None, ep, qp, oep, obp, orp), (idx.h, ests, None, qp, oep, obp, orp),
                 (idx.h, ests, ep, None, oep, obp, orp), (idx.h, ests, ep, qp, None, obp, orp), (idx.h, ests, ep, qp, oep, None, orp),
                 (idx.h, ests, ep, qp, oep, obp, None)):
        ih, es, e_, q_, oe_, ob_, or_ = args
        assert f(gpu_ctx.h, ih, es, len(ests), e_, n_ex, q_, len(q), pp, oe_, ob_, or_) == capi.PGPU_EINVAL
        assert L.pgpu_last_error(gpu_ctx.h).decode() == MESSAGE                   # of the refusal before: untouched
        assert idx.small_chains_kernel_ms() == 0.0
    assert f(None, idx.h, ests, len(ests), ep, n_ex, qp, len(q), pp, oep, obp, orp) == capi.PGPU_EINVAL
    check(idx, ests, exons, q, 60, want)
    assert idx.small_chains_kernel_ms() > 0.0
    assert f(gpu_ctx.h, idx.h, ests, len(ests), ep, n_ex, None, 0, pp, oep, obp, None) == capi.PGPU_OK   # n == 0: every slot 0
    assert not oe.tobytes().strip(b"\0") and not ob.any() and idx.small_chains_kernel_ms() == 0.0
    assert f(gpu_ctx.h, idx.h, None, 0, None, 0, None, 0, pp, None, None, None) == capi.PGPU_OK
    check(idx, ests, exons, q, 60, want)                                          # the context still answers


def test_without_timing_the_answers_are_the_same(golden):
    import pintron_amd.capi as capi
    gen, cases, _ = golden
    part = [c for c in cases if c["mil"] == 60][:120]
    ests, exons, q = SL.batch_arrays(SL.quints(part))
    want = SL.expect_arrays(exons, q, answers(part))
    with capi.Context(0) as ctx:
        idx = capi.Index(ctx, gen)
        check(idx, ests, exons, q, 60, want)
        assert idx.small_chains_kernel_ms() > 0.0
        ctx.L.pgpu_set_timing(ctx.h, 0)
        check(idx, ests, exons, q, 60, want)
        assert idx.small_chains_kernel_ms() == 0.0
        idx.close()
