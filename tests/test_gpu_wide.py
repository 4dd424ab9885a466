"""GPU: the wide entries -- pgpu_index_tail_chains_wide, pgpu_index_small_chains_wide, pgpu_index_final_factorizations_wide
and pgpu_pairing_plan_run_final_factorizations_wide -- against the fixture that the reference's object code, the wide
restatement and the host code agreed on (tests/golden/wide_chains.json.gz), against the narrow entries wherever those
answer, and against the wide restatement (tests/wide_lib.py).  Every comparison is byte equality: results, exons, step
bytes."""
import ctypes as C
import os

import numpy as np
import pytest

import cand_lib as KL
import fact_lib as F
import final_lib as FL
import meg_lib as M
import small_lib as SL
import tail_lib as TL
import unit_lib as UL
import wide_lib as WL

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same(got, want, what=""):
    for name, g, w in zip(("first", "second", "third"), got, want):
        assert len(g) == len(w), (what, name, len(g), len(w))
        if bytes(g) != bytes(w):                                   # (a numpy array, or the bytes of a blob)
            bad = [i for i in range(len(g)) if g[i] != w[i]]
            raise AssertionError("%s: the %s arrays differ at %d places, first %d: %r / %r" % (what, name, len(bad), bad[0], g[bad[0]], w[bad[0]]))


def tail_batch(cases):
    ests, exons, q = TL.batch_arrays(TL.quads(cases))
    return ests, exons, q, TL.expect_arrays(exons, [c["answer"] for c in cases])


def small_batches(cases):
    """one batch per min_intron_length: (mil, ests, exons, q, expected arrays)"""
    out = []
    for mil in sorted({c["mil"] for c in cases}):
        group = [c for c in cases if c["mil"] == mil]
        ests, exons, q = SL.batch_arrays(SL.quints(group))
        out.append((mil, ests, exons, q, SL.expect_arrays(exons, q, [c["answer"] for c in group])))
    return out


@pytest.fixture(scope="module")
def golden(gpu_ctx):
    import pintron_amd.capi as capi
    gen, tails, smalls = WL.load_fixture()
    idx = capi.Index(gpu_ctx, gen)
    yield gen, tails, smalls, idx
    idx.close()


@pytest.fixture(scope="module")
def neighbours():
    """ordinary cases over the fixture's sequence with the wide restatement's answers, which are the narrow one's"""
    gen = WL.load_fixture()[0]
    tails, smalls = WL.make_world()[3]
    ops = SL.OracleOps(gen)
    t = [dict(name=n, orig=o, est=e, exons=x, answer=WL.tail(o, e, gen, x)) for n, o, e, x in tails]
    s = [dict(name=n, orig=o, est=e, exons=x, mil=m, answer=WL.small(o, e, gen, x, m, ops=ops)) for n, o, e, x, m in smalls]
    assert all(c["answer"][0] == TL.OK and c["answer"] == TL.tail(c["orig"], c["est"], gen, c["exons"]) for c in t)
    assert all(c["answer"][0] == SL.OK for c in s)
    return t, s


# ---- the two chained entries ------------------------------------------------------------------------------------------
def test_the_fixture_through_the_two_wide_entries_built_reloaded_and_twice(golden, gpu_ctx, tmp_path):
    import pintron_amd.capi as capi
    gen, tails, smalls, idx = golden
    path = str(tmp_path / "wide.idx")
    idx.save(path)
    loaded = capi.Index(gpu_ctx, gen, load_from=path)
    try:
        ests, exons, q, want = tail_batch(tails)
        first = idx.tail_chains(ests, exons, q, wide=True)
        same(first, want, "tail")
        assert idx.tail_chains_kernel_ms() > 0.0                   # the narrow entry's getter reports the wide call
        same(idx.tail_chains(ests, exons, q, wide=True), first, "tail again")
        r_ests, r_exons, r_q, r_want = tail_batch(tails[::-1])
        same(idx.tail_chains(r_ests, r_exons, r_q, wide=True), r_want, "tail, every case in reverse")
        same(loaded.tail_chains(ests, exons, q, wide=True), want, "tail, loaded")
        # the narrow entry on the same batch: PGPU_ERANGE wherever a wide window's DP runs, else the same bytes
        narrow = idx.tail_chains(ests, exons, q)[2]
        for i, c in enumerate(tails):
            if c["tags"] & {"pre_wide", "suf_wide"}:
                assert narrow["status"][i] == TL.ERANGE, c["name"]
            else:
                assert narrow[i] == want[2][i], c["name"]
        for mil, ests, exons, q, want in small_batches(smalls):
            first = idx.small_chains(ests, exons, q, mil, wide=True)
            same(first, want, "small")
            assert idx.small_chains_kernel_ms() > 0.0
            same(idx.small_chains(ests, exons, q, mil, wide=True), first, "small again")
        for mil, ests, exons, q, want in small_batches(smalls[::-1]):
            same(idx.small_chains(ests, exons, q, mil, wide=True), want, "small, every case in reverse")
        for mil, ests, exons, q, want in small_batches(smalls):
            same(loaded.small_chains(ests, exons, q, mil, wide=True), want, "small, loaded")
    finally:
        loaded.close()


def test_the_narrow_fixtures_through_the_wide_entries_equal_the_narrow_entries(gpu_ctx):
    import pintron_amd.capi as capi
    gen, cases, _ = TL.load_fixture()
    idx = capi.Index(gpu_ctx, gen)
    try:
        ests, exons, q = TL.batch_arrays(TL.quads(cases))
        narrow, wide = idx.tail_chains(ests, exons, q), idx.tail_chains(ests, exons, q, wide=True)
        n = 0
        for i, c in enumerate(cases):
            lo, k = int(q["first_exon"][i]), int(q["n_exons"][i])
            if narrow[2]["status"][i] == TL.OK:
                assert wide[2][i] == narrow[2][i], c["name"]
                assert wide[0][lo:lo + k].tobytes() == narrow[0][lo:lo + k].tobytes(), c["name"]
                assert wide[1][lo:lo + k].tobytes() == narrow[1][lo:lo + k].tobytes(), c["name"]
                n += 1
        assert n >= 400 and (narrow[2]["status"] != TL.OK).sum() > (wide[2]["status"] != TL.OK).sum() > 0
    finally:
        idx.close()
    for g, cases in SL.load_fixture()[0]:
        idx = capi.Index(gpu_ctx, g)
        try:
            for mil, ests, exons, q, want in small_batches(cases):
                narrow, wide = idx.small_chains(ests, exons, q, mil), idx.small_chains(ests, exons, q, mil, wide=True)
                for i in range(len(q)):
                    lo, k = 2 * int(q["first_exon"][i]), 2 * int(q["n_exons"][i])
                    if narrow[2]["refused"][i] != 2:
                        assert wide[2][i] == narrow[2][i], (mil, i)
                        assert wide[0][lo:lo + k].tobytes() == narrow[0][lo:lo + k].tobytes(), (mil, i)
                        assert wide[1][lo:lo + k].tobytes() == narrow[1][lo:lo + k].tobytes(), (mil, i)
                    else:
                        assert wide[2]["refused"][i] != 2, (mil, i)
        finally:
            idx.close()


def picked(cases, tags):
    """the first case of each tag, each once"""
    out = []
    for t in tags:
        c = next(c for c in cases if t in c["tags"])
        if not any(c is o for o in out):
            out.append(c)
    return out


def test_hand_made_cases_between_ordinary_neighbours_in_reverse_and_one_by_one(golden, neighbours):
    gen, tails, smalls, idx = golden
    nt, ns = neighbours
    some = picked(tails, WL.TAIL_TAGS) + [c for c in tails if c["tags"] & {"affix_257", "affix_1024"}][:8] + \
        [c for c in tails if c["answer"][0] == TL.ERANGE][:6]
    batch = []
    for k, c in enumerate(some):
        batch += [nt[k % len(nt)], c]
    batch.append(nt[0])
    for order in (batch, batch[::-1]):
        ests, exons, q, want = tail_batch(order)
        same(idx.tail_chains(ests, exons, q, wide=True), want, "tail between neighbours")
        refused = want[2]["status"] == TL.ERANGE
        assert refused.sum() >= 3
        for i in np.flatnonzero(refused):                          # as the narrow entry refuses: the exons untouched, everything else 0
            lo, n = int(q[i]["first_exon"]), int(q[i]["n_exons"])
            assert want[0][lo:lo + n].tobytes() == exons[lo:lo + n].tobytes() and not want[1][lo:lo + n].any()
            assert bytes(want[2][i].tobytes()[4:]) == bytes(12)
    for c in some:
        ests, exons, q, want = tail_batch([c])
        same(idx.tail_chains(ests, exons, q, wide=True), want, c["name"])
    some = picked(smalls, WL.SMALL_TAGS) + [c for c in smalls if c["tags"] & {"window_1024", "window_1025", "window_257"}][:12]
    batch = []
    for k, c in enumerate(some):
        batch += [ns[k % len(ns)], c]
    batch.append(ns[0])
    for order in (batch, batch[::-1]):
        for mil, ests, exons, q, want in small_batches(order):
            same(idx.small_chains(ests, exons, q, mil, wide=True), want, "small between neighbours")
            assert set(want[2]["refused"].tolist()) >= {0, 2, 4}
    for c in some:
        for mil, ests, exons, q, want in small_batches([c]):
            same(idx.small_chains(ests, exons, q, mil, wide=True), want, c["name"])


def test_batches_of_1_255_256_and_257_with_one_wide_query_and_a_batch_of_wide_ones(golden, neighbours):
    gen, tails, smalls, idx = golden
    nt, ns = neighbours
    wide_t = [c for c in tails if c["tags"] & {"pre_wide", "suf_wide"} and c["answer"][0] == TL.OK]
    wide_s = [c for c in smalls if c["tags"] & {"wide_inserted", "wide_not_inserted"}]
    assert len(wide_t) >= 60 and len(wide_s) >= 60
    for n in (1, 255, 256, 257):
        at = (n * 5) // 7
        batch = [nt[k % len(nt)] for k in range(n)]
        batch[at] = wide_t[n % len(wide_t)]
        ests, exons, q, want = tail_batch(batch)
        same(idx.tail_chains(ests, exons, q, wide=True), want, ("tail", n))
        batch = [ns[k % len(ns)] for k in range(n)]
        batch[at] = wide_s[n % len(wide_s)]
        for mil, ests, exons, q, want in small_batches(batch):
            same(idx.small_chains(ests, exons, q, mil, wide=True), want, ("small", n))
    ests, exons, q, want = tail_batch(wide_t)
    same(idx.tail_chains(ests, exons, q, wide=True), want, "every query wide")
    assert (idx.tail_chains(ests, exons, q)[2]["status"] == TL.ERANGE).all()
    for mil, ests, exons, q, want in small_batches(wide_s):
        same(idx.small_chains(ests, exons, q, mil, wide=True), want, "every query wide")
        assert (idx.small_chains(ests, exons, q, mil)[2]["refused"] == 2).all()


def test_the_refusals_of_the_narrow_entries_answered_alike(golden, neighbours, gpu_ctx):
    import pintron_amd.capi as capi
    gen, tails, smalls, idx = golden
    L_ = gpu_ctx.L
    cases = neighbours[0] + tails[:6]
    ests, exons, q, _ = tail_batch(cases)

    def both(call):
        """(rc, message) of the narrow and of the wide form of one call"""
        out = []
        for wide in (False, True):
            rc = call(wide)
            out.append((rc, L_.pgpu_last_error(gpu_ctx.h).decode() if rc != capi.PGPU_OK else ""))
        assert out[0] == out[1], out
        return out[0]

    mid = 4
    changes = [("reserved", 1), ("est_len", 0), ("est_off", len(ests)), ("est_len", len(ests) + 1), ("first_exon", len(exons)),
               ("n_exons", 0), ("n_exons", len(exons) + 1), ("first_exon", int(q["first_exon"][mid]) - 1),
               ("orig_off", len(ests)), ("orig_off", (1 << 64) - 1)]
    for field, value in changes:
        q2 = q.copy()
        q2[field][mid] = value
        rc, msg = both(lambda wide: idx.tail_chains_raw(ests, exons, q2, len(q2), wide=wide)[0])
        assert rc == capi.PGPU_EINVAL and msg.startswith("bad tail query"), (field, value, rc, msg)
        rc, msg = both(lambda wide: idx.small_chains_raw(ests, exons, q2, len(q2), 40, wide=wide)[0])
        assert rc == capi.PGPU_EINVAL and msg.startswith("bad small query"), (field, value, rc, msg)
    ex2 = exons.copy()
    ex2[int(q["first_exon"][mid])] = (0, int(q["est_len"][mid]), 0, 0)               # a coordinate that is no byte of the EST
    assert both(lambda wide: idx.tail_chains_raw(ests, ex2, q, len(q), wide=wide)[0])[0] == capi.PGPU_EINVAL
    assert both(lambda wide: idx.small_chains_raw(ests, ex2, q, len(q), 40, wide=wide)[0])[0] == capi.PGPU_EINVAL
    rc, msg = both(lambda wide: idx.small_chains_raw(ests, exons, q, len(q), 40, params_reserved=1, wide=wide)[0])
    assert rc == capi.PGPU_EINVAL and "reserved" in msg
    assert both(lambda wide: idx.small_chains_raw(ests, exons, q, len(q), 40, no_params=True, wide=wide)[0])[0] == capi.PGPU_EINVAL
    # null pointers: a bare refusal
    out_ex = np.zeros(len(exons), dtype=exons.dtype)
    out_st = np.zeros(len(exons), dtype=np.uint8)
    res = np.zeros(len(q), dtype=np.dtype(capi.TAIL_RESULT_DTYPE))
    full = [gpu_ctx.h, idx.h, ests, len(ests), exons.ctypes.data_as(C.POINTER(capi.Factor)), len(exons),
            q.ctypes.data_as(C.POINTER(capi.TailQuery)), len(q), out_ex.ctypes.data_as(C.POINTER(capi.Factor)),
            out_st.ctypes.data_as(C.POINTER(C.c_uint8)), res.ctypes.data_as(C.POINTER(capi.TailResult))]
    for k in (0, 1, 2, 4, 6, 8, 9, 10):
        args = list(full)
        args[k] = None
        assert L_.pgpu_index_tail_chains(*args) == L_.pgpu_index_tail_chains_wide(*args) == capi.PGPU_EINVAL, k
    # n == 0: PGPU_OK, the exons copied, the steps 0; and the context still answers
    for wide in (False, True):
        rc, oe, os_, _ = idx.tail_chains_raw(ests, exons, q[:0], 0, wide=wide)
        assert rc == capi.PGPU_OK and oe.tobytes() == exons.tobytes() and not os_.any()
        rc, oe, os_, _ = idx.small_chains_raw(ests, exons, q[:0], 0, 40, wide=wide)
        assert rc == capi.PGPU_OK and not oe.view(np.uint8).any() and not os_.any()
    ests, exons, q, want = tail_batch(cases)
    same(idx.tail_chains(ests, exons, q, wide=True), want, "afterwards")


# ---- the final stage --------------------------------------------------------------------------------------------------
def final_device(idx, ests, exons, q, prm, mil, wide):
    import pintron_amd.capi as capi
    rc, res, ex, st, total = idx.final_factorizations_raw(ests, exons, q, len(q), capi.FactParams(*prm), capi.SmallParams(mil, 0),
                                                          2 * len(exons), wide=wide)
    idx.ctx.check(rc)
    return res, ex[:total], st[:total]


def triples(cases):
    return [(c["orig"], c["est"], c["exons"]) for c in cases]


def test_the_wide_final_form_on_the_hand_made_cases_flips_host_to_done(gpu_ctx):
    """The test that cannot pass without the wide kernels: the cases of final_lib tagged tail_affix_257 and
    small_window_257 are HOST under pgpu_index_final_factorizations and DONE, with the wide restatement's exons, under
    pgpu_index_final_factorizations_wide; every other case is the same bytes under both."""
    import pintron_amd.capi as capi
    flipped = {"tail_affix_257": 0, "small_window_257": 0}
    for name, g, cases in FL.hand_groups():
        idx = capi.Index(gpu_ctx, g)
        ops = SL.OracleOps(g)
        try:
            for (prm, mil), group in FL.by_settings(cases).items():
                ests, exons, q = FL.batch_arrays(triples(group))
                narrow = final_device(idx, ests, exons, q, prm, mil, False)
                same(narrow, FL.expect_arrays([c["answer"] for c in group]), (name, "narrow"))
                wide_answers = []
                for c in group:
                    hit = c["tags"] & set(flipped)
                    a = c["answer"]
                    if hit:
                        a = WL.final(KL.ONE if c["exons"] else KL.NONE, c["orig"], c["est"], g, c["exons"], c["prm"], c["mil"], ops=ops)
                    for t in hit:
                        assert c["answer"]["outcome"] == FL.HOST and c["answer"]["detail"] == 1, c["name"]
                        assert a["outcome"] == FL.DONE and a["exons"], (c["name"], a)
                        flipped[t] += 1
                    wide_answers.append(a)
                wide = final_device(idx, ests, exons, q, prm, mil, True)
                same(wide, FL.expect_arrays(wide_answers), (name, "wide"))
                assert idx.final_factorizations_kernel_ms() > 0.0
                for i, c in enumerate(group):
                    if c["tags"] & set(flipped):
                        assert narrow[0]["outcome"][i] == FL.HOST and wide[0]["outcome"][i] == FL.DONE, c["name"]
                    else:
                        a, b = narrow[0][i:i + 1].copy(), wide[0][i:i + 1].copy()
                        a["first_exon"], b["first_exon"] = 0, 0
                        assert a.tobytes() == b.tobytes(), c["name"]
        finally:
            idx.close()
    assert min(flipped.values()) >= 1, flipped


def units_keep_their_bytes(narrow_units, wide_units):
    """every unit the narrow finals settle has the same verdict and the same record bytes under the wide ones -> the units
    that were HOST and are settled now"""
    (nu, nb), (wu, wb) = narrow_units, wide_units
    flipped = []
    for i in range(len(nu)):
        if int(nu["verdict"][i]) == UL.U_HOST:
            if int(wu["verdict"][i]) != UL.U_HOST:
                flipped.append(i)
            continue
        a, b = nu[i:i + 1].copy(), wu[i:i + 1].copy()
        a["first_byte"], b["first_byte"] = 0, 0
        assert a.tobytes() == b.tobytes(), i
        assert nb[int(nu["first_byte"][i]):int(nu["first_byte"][i]) + int(nu["n_bytes"][i])] == \
            wb[int(wu["first_byte"][i]):int(wu["first_byte"][i]) + int(wu["n_bytes"][i])], i
    return flipped


def run_plan(plan, prm, wide, mil=40):
    plan.run(prm["min_factor_len"], 0.2)
    plan.run_meg(**prm)
    plan.run_candidates(prm["min_factor_len"], prm["min_intron_length"])
    plan.run_factorizations(*F.DEFAULTS)
    plan.run_final_factorizations(mil, wide=wide)
    return plan.fetch_final_factorizations()


@pytest.mark.parametrize("source,n_pat", [("c2", 307), ("issue13", 1891)])
@pytest.mark.parametrize("resident", [False, True])
def test_plan_form_against_the_wide_restatement_the_wide_index_form_and_units_on_top(gpu_ctx, tmp_path, source, n_pat, resident):
    import pintron_amd.capi as capi
    U = UL.real_units(source)
    seqs, genomic = U["working"], U["genomic"]
    assert len(seqs) == n_pat
    originals = {k: o for k, (w, o) in enumerate(zip(seqs, U["original"])) if o != w}
    uq = UL.unit_queries(U)
    idx = capi.Index(gpu_ctx, genomic)
    plan = capi.PairingPlan(gpu_ctx, idx, seqs, resident=resident, originals=originals)
    ops = SL.OracleOps(genomic)
    try:
        narrow = run_plan(plan, M.DEFAULTS, False)
        plan.run_units(uq, U["pref_N"], 1)
        narrow_units = plan.fetch_units()
        got = run_plan(plan, M.DEFAULTS, True)
        assert all(plan.final_ms(k) > 0.0 for k in range(3))
        cres, cex = plan.fetch_candidates()
        mine = []
        for k in range(n_pat):
            lo, n = int(cres["first_exon"][k]), int(cres["n_exons"][k])
            mine.append(WL.final(int(cres["kind"][k]), originals.get(k, seqs[k]), seqs[k], genomic,
                                 [tuple(int(v) for v in e) for e in cex[lo:lo + n]], ops=ops))
        same(got, FL.expect_arrays(mine), source + " the wide restatement")
        # the wide index form fed with the fetched candidates
        off = np.zeros(n_pat + 1, dtype=np.uint64)
        np.cumsum([len(s) for s in seqs], out=off[1:])
        orig_off = off[:-1].copy()
        blob, at = b"".join(seqs), int(off[-1])
        for k in sorted(originals):
            orig_off[k] = at
            at += len(originals[k])
        blob += b"".join(originals[k] for k in sorted(originals))
        q = FL.plan_queries(off, cres, orig_off)
        r2, e2, s2 = final_device(idx, blob, cex, q, F.DEFAULTS, 40, True)
        same(got, (FL.stage0_of_kinds(r2, cres["kind"]), e2, s2), source + " the wide index form")
        # a rerun gives the same bytes; units on top: a unit the narrow finals settle does not change a byte
        plan.run_final_factorizations(40, wide=True)
        same(plan.fetch_final_factorizations(), got, "a rerun")
        host_narrow = narrow[0]["outcome"] == FL.HOST
        settled = ~host_narrow
        assert (got[0]["outcome"][settled] == narrow[0]["outcome"][settled]).all()
        plan.run_units(uq, U["pref_N"], 1)
        wide_units = plan.fetch_units()
        flips = int((host_narrow & (got[0]["outcome"] != FL.HOST)).sum())
        nr = narrow[0]
        for_window = host_narrow & (nr["detail"] == 1) & ((nr["stage"] == 4) | ((nr["stage"] == 5) & (nr["refused"] == 2)))
        if flips == 0:                                                 # no record leaves HOST: one that met a window cap may meet
            keep = np.flatnonzero(~for_window)                         # another cap further on, every other result is the same
            same((got[0][keep], got[1], got[2]), (nr[keep], narrow[1], narrow[2]), "no flip: the narrow finals")
            same(wide_units, narrow_units, "no flip: the narrow units")
        else:
            assert (got[0][~for_window]["outcome"] == nr[~for_window]["outcome"]).all()
        units_keep_their_bytes(narrow_units, wide_units)
        gfa, efa = KL.real_inputs()[source]
        product = UL.program_records(os.path.join(ROOT, "pintron_amd", "bin", "est-fact"), gfa, efa, 1, str(tmp_path))
        n_aligned, n_unaligned, wrong = UL.against_the_program(wide_units[0], wide_units[1], uq, product)
        assert not wrong and n_aligned > 0, (n_aligned, n_unaligned, wrong[:10])
    finally:
        plan.close()
        idx.close()


# ---- one end-to-end case with flips that are certain ----------------------------------------------------------------------
# Chosen on the CPU with the restatements (unit_lib.finals under wide_lib.caps, then unit_lib.units).  synth.py's C2 shape
# (ESTs of 500 +- 100 bases, 1 % errors) has too few: seeds 1, 2, 3, 5, 7, 11 at 3 000 to 5 000 ESTs give 5, 1, 3, 2, 6 and 0
# units that are HOST for a window cap under the narrow finals and settled under the wide ones, one in a thousand, so no
# workload of a few thousand ESTs reaches 20.  The C3 shape (600 +- 100 bases, 3 % errors), whose chunk DESIGN.md section 5r
# measures, has them: 400 ESTs at seed 1 give 37 (36 ALIGNED, 1 UNALIGNED), 15 HOST units left of 52.
E2E_SHAPE, E2E_ESTS, E2E_SEED, E2E_FLIPS = "C3", 400, 1, 37


def test_end_to_end_the_flipped_units_of_a_synthetic_workload_equal_the_product(gpu_ctx, tmp_path):
    import pintron_amd.capi as capi
    import side_lib as SIDE
    import text_lib as TXT
    from pintron_amd import synth
    w = synth.make(E2E_SHAPE, n_est=E2E_ESTS, seed=E2E_SEED)
    gfa, efa = w.genomic_fasta(), w.ests_fasta()
    U = UL.prepared(gfa, efa)
    seqs, genomic = U["working"], U["genomic"]
    originals = {k: o for k, (wk, o) in enumerate(zip(seqs, U["original"])) if o != wk}
    q = UL.unit_queries(U)
    ids = TXT.est_headers(efa)
    headers = [ids[int(i)] for i in q["est_index"]]
    # the product, once: its records, its two text files and its three side files, cut per EST
    d = str(tmp_path / "product")
    rec, raw, pests = TXT.program_texts(os.path.join(ROOT, "pintron_amd", "bin", "est-fact"), gfa, efa, 1, d)
    groups = UL.groups_by_index(rec)
    their_texts = TXT.per_est(rec, raw, pests)
    their_sides = SIDE.per_est(ids, *SIDE.program_sides(d))
    idx = capi.Index(gpu_ctx, genomic)
    src = capi.TextSource(gpu_ctx, TXT.original_genomic(gfa))
    plan = capi.PairingPlan(gpu_ctx, idx, seqs, resident=True, originals=originals)
    try:
        narrow = run_plan(plan, M.DEFAULTS, False)
        plan.run_units(q, U["pref_N"], 1)
        narrow_units = plan.fetch_units()
        wide = run_plan(plan, M.DEFAULTS, True)
        plan.run_units(q, U["pref_N"], 1)
        units, blob = plan.fetch_units()
        flipped = units_keep_their_bytes(narrow_units, (units, blob))
        nr = narrow[0]
        for_window = (nr["outcome"] == FL.HOST) & (nr["detail"] == 1) & ((nr["stage"] == 4) | ((nr["stage"] == 5) & (nr["refused"] == 2)))
        assert (wide[0][~for_window]["outcome"] == nr[~for_window]["outcome"]).all()
        print("flipped units: %d (the restatement: %d)" % (len(flipped), E2E_FLIPS))
        assert len(flipped) == E2E_FLIPS >= 20, len(flipped)
        plan.run_texts(src, headers)
        texts = plan.fetch_texts()
        plan.run_sides()
        sides = plan.fetch_sides()
        n_aligned = 0
        for i in flipped:
            e = int(q["est_index"][i])
            # a flip is a pattern that met a window cap: the unit's forward pattern or its sibling
            assert for_window[int(q["fwd"][i])] or (int(q["rev"][i]) != UL.NO_SIBLING and for_window[int(q["rev"][i])]), i
            at, n = int(units["first_byte"][i]), int(units["n_bytes"][i])
            if int(units["verdict"][i]) == UL.U_ALIGNED:
                n_aligned += 1
                assert groups.get(e) == blob[at:at + n], (i, e)
                a, n1, b, n2 = (int(texts[0][f][i]) for f in ("raw_first", "raw_bytes", "pests_first", "pests_bytes"))
                assert int(texts[0]["verdict"][i]) == TXT.DONE and their_texts[e] == (texts[1][a:a + n1], texts[2][b:b + n2]), (i, e)
            else:
                assert e not in groups, (i, e)
            assert int(sides[0]["verdict"][i]) == SIDE.DONE, i
            mine = tuple(sides[1 + k][int(sides[0][f + "_first"][i]):int(sides[0][f + "_first"][i]) + int(sides[0][f + "_bytes"][i])]
                         for k, f in enumerate(("megs", "pmegs", "edges")))
            assert their_sides[e] == mine, (i, e)
        assert n_aligned >= 20, n_aligned
        # and every settled unit, flipped or not, against the product's records
        _, _, wrong = UL.against_the_program(units, blob, q, rec)
        assert not wrong, wrong[:10]
    finally:
        plan.close()
        src.close()
        idx.close()
