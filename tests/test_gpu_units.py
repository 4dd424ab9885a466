"""GPU: the unit stage (pgpu_unit_records, pgpu_pairing_plan_run_units) byte for byte against its restatement
(tests/unit_lib.py) -- the form without a plan on the hand-made cases in batches around the block and the scan's tile, every
refusal, with and without timing; the plan form on c2 and test-issue-13, plain and resident, against the restatement on the
device's own finals and record headers, against the form without a plan on the same arrays, and against the records the
product binary writes for the same files; the sixth rung's rules."""
import ctypes as C
import os

import numpy as np
import pytest

import cand_lib as KL
import fact_lib as F
import final_lib as FL
import meg_lib as M
import unit_lib as UL
from test_unit_cpu import FLOORS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def message(ctx):
    return ctx.L.pgpu_last_error(ctx.h).decode()


def device(ctx, res, exons, empty, q, pref_N=0, retain=1):
    import pintron_amd.capi as capi
    return capi.unit_records(ctx, res, exons, empty, q, pref_N, retain)


def same(got, want, what=""):
    assert got[0].dtype == want[0].dtype and len(got[0]) == len(want[0]), what
    for f in got[0].dtype.names:
        bad = np.nonzero(got[0][f] != want[0][f])[0]
        assert len(bad) == 0, (what, f, int(bad[0]), got[0][int(bad[0])], want[0][int(bad[0])])
    assert got[1] == want[1], what


@pytest.fixture(scope="module")
def hand():
    return UL.batch(UL.hand_cases())


@pytest.mark.parametrize("pref_N,retain", UL.SETTINGS)
def test_hand_made_cases_in_one_batch_in_reverse_and_one_by_one(gpu_ctx, hand, pref_N, retain):
    res, exons, empty, q = hand
    want = UL.units(res, exons, empty, q, pref_N, retain)
    same(device(gpu_ctx, res, exons, empty, q, pref_N, retain), want, "one batch")
    assert gpu_ctx.L.pgpu_unit_records_kernel_ms() > 0.0
    back = q[::-1].copy()
    same(device(gpu_ctx, res, exons, empty, back, pref_N, retain), UL.units(res, exons, empty, back, pref_N, retain), "in reverse")
    for i in range(len(q)):
        out, blob = device(gpu_ctx, res, exons, empty, q[i:i + 1], pref_N, retain)
        at, n = int(want[0]["first_byte"][i]), int(want[0]["n_bytes"][i])
        assert blob == want[1][at:at + n] and int(out["first_byte"][0]) == 0, i
        one = want[0][i:i + 1].copy()
        one["first_byte"] = 0
        assert out.tobytes() == one.tobytes(), (i, out, one)
    # no empty-graph bytes at all: none is empty
    same(device(gpu_ctx, res, exons, None, q, pref_N, retain), UL.units(res, exons, None, q, pref_N, retain), "no bytes")


def repeated(n):
    """n units made by repeating the hand-made cases, each copy with patterns of its own"""
    cases = UL.hand_cases()
    reps = [dict(cases[k % len(cases)], est_index=(7919 * k) & 0xffffffff) for k in range(n)]
    return UL.batch(reps, seed=n)


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 2047, 2048, 2049])
def test_batches_around_the_block_and_the_scan_tile(gpu_ctx, n):
    res, exons, empty, q = repeated(max(n, 1))
    q = q[:n]
    for pref_N, retain in ((0, 1), (77, 0)):
        same(device(gpu_ctx, res, exons, empty, q, pref_N, retain), UL.units(res, exons, empty, q, pref_N, retain), (n, retain))


def test_a_batch_without_an_aligned_unit_and_results_that_share_exons(gpu_ctx, hand):
    res, exons, empty, q = hand
    want = UL.units(res, exons, empty, q)
    none = q[want[0]["verdict"] != UL.U_ALIGNED]
    assert len(none) > 30
    out, blob = device(gpu_ctx, res, exons, empty, none)
    assert blob == b"" and not out["n_bytes"].any() and not out["first_byte"].any()
    same((out, blob), UL.units(res, exons, empty, none))
    # 40 results over the same four exons: the blob is larger than the exon array
    shared = np.zeros(40, dtype=res.dtype)
    shared["outcome"], shared["stage"], shared["n_exons"], shared["polyA"] = FL.DONE, 5, 4, 1
    ex4 = np.array(UL._exons((30, 40, 50, 60)), dtype=exons.dtype)
    qs = UL.query_array([(k, k, UL.NO_SIBLING, 0) for k in range(40)])
    got = device(gpu_ctx, shared, ex4, None, qs, 5, 1)
    same(got, UL.units(shared, ex4, None, qs, 5, 1))
    assert len(got[1]) == 40 * (12 + 64) > 16 * len(ex4)


def test_every_refusal_and_enospc(gpu_ctx, hand):
    import pintron_amd.capi as capi
    res, exons, empty, q = hand
    want = UL.units(res, exons, empty, q)
    n, total = len(q), len(want[1])

    def call(res=res, exons=exons, empty=empty, q=q, n=n, prm=None, cap=total, n_pat=None):
        rc, out, blob, length = capi.unit_records_raw(gpu_ctx, res, exons, empty, q, n, capi.unit_params() if prm is None else prm, cap, n_pat)
        if rc != capi.PGPU_OK:
            assert not out.view(np.uint8).any() and not blob.any()                    # nothing written
            assert gpu_ctx.L.pgpu_unit_records_kernel_ms() == 0.0
        return rc, length

    assert call() == (capi.PGPU_OK, total)

    def refused(text, **kw):
        rc, _ = call(**kw)
        return rc == capi.PGPU_EINVAL and text in message(gpu_ctx)

    def changed(field, i, value, arr=q):
        a = arr.copy()
        a[field][i] = value
        return a
    paired = int(np.nonzero(q["rev"] != UL.NO_SIBLING)[0][0])
    assert refused("fwd is no pattern", q=changed("fwd", 3, len(res)))
    assert refused("fwd is no pattern", q=changed("fwd", 3, UL.NO_SIBLING))
    assert refused("rev is neither", q=changed("rev", 3, len(res)))
    assert refused("rev is neither", q=changed("rev", 3, UL.NO_SIBLING - 1))
    assert refused("fwd == rev", q=changed("rev", 3, int(q["fwd"][3])))
    assert refused("named by two units", q=changed("fwd", 3, int(q["fwd"][9])))
    assert refused("named by two units", q=changed("rev", 3, int(q["fwd"][9])))
    assert refused("named by two units", q=changed("fwd", n - 1, int(q["rev"][paired])))
    assert refused("flag bits", q=changed("flags", 5, 4))
    assert refused("flag bits", q=changed("flags", 5, 1 << 31))
    assert refused("reserved != 0", prm=capi.unit_params(0, 1, (0, 0, 1)))
    assert refused("reserved != 0", prm=capi.unit_params(0, 1, (1, 0, 0)))
    assert refused("retain_externals above 1", prm=capi.unit_params(0, 2))
    assert refused("pref_N_length outside", prm=capi.unit_params(-1, 1))
    assert refused("pref_N_length outside", prm=capi.unit_params((1 << 30) + 1, 1))
    assert call(prm=capi.unit_params(1 << 30, 1))[0] == capi.PGPU_OK
    done = int(np.nonzero(res["outcome"] == FL.DONE)[0][0])
    last = int(np.argmax(res["first_exon"].astype(np.int64) + res["n_exons"]))
    assert refused("an outcome above 2", res=changed("outcome", 7, 3, res))
    assert refused("an outcome above 2", res=changed("outcome", 7, 255, res))
    assert refused("n_exons == 0 or above 128", res=changed("n_exons", done, 0, res))
    assert refused("n_exons == 0 or above 128", res=changed("n_exons", done, 129, res))
    assert refused("beyond the exons", res=changed("first_exon", last, int(res["first_exon"][last]) + 1, res))
    assert refused("beyond the exons", res=changed("first_exon", done, 0xffffffff, res))
    assert refused("beyond the exons", exons=exons[:-1])
    assert refused("more than 2^31 - 1", n=1 << 31)                                    # counts alone: no unit is read
    assert refused("more than 2^31 - 1", n_pat=1 << 31, n=0)
    # a refused result that no unit names is refused all the same: the rule is on the call
    unnamed = np.concatenate([res, changed("outcome", 0, 9, res[:1])])
    assert refused("an outcome above 2", res=unnamed, empty=np.concatenate([empty, empty[:1]]))
    # null pointers: a bare PGPU_EINVAL
    L_ = gpu_ctx.L
    p = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    out = np.zeros(n, dtype=np.dtype(capi.UNIT_RESULT_DTYPE))
    blob = np.zeros(total, dtype=np.uint8)
    length = C.c_size_t(0)
    prm = capi.unit_params()
    args = [gpu_ctx.h, p(res, capi.FinalResult), len(res), p(exons, capi.Factor), len(exons), p(empty, C.c_uint8), p(q, capi.UnitQuery), n,
            C.byref(prm), p(out, capi.UnitResult), blob.ctypes.data_as(C.c_void_p), total, C.byref(length)]
    assert L_.pgpu_unit_records(*args) == capi.PGPU_OK
    for k in (0, 1, 3, 6, 8, 9, 10, 12):
        a = list(args)
        a[k] = None
        assert L_.pgpu_unit_records(*a) == capi.PGPU_EINVAL, k
    a = list(args)
    a[5] = None                                                                       # no empty-graph bytes: a value
    assert L_.pgpu_unit_records(*a) == capi.PGPU_OK
    # PGPU_ENOSPC with its count, nothing written; n == 0
    for cap in (0, 4, total - 4, total - 1):
        rc, length = call(cap=cap)
        assert rc == capi.PGPU_ENOSPC and length == total and message(gpu_ctx) == "blob too small", cap
    assert call(q=q[:0], n=0) == (capi.PGPU_OK, 0)
    assert call(q=q[:0], n=0, cap=0) == (capi.PGPU_OK, 0)
    assert refused("retain_externals above 1", q=q[:0], n=0, prm=capi.unit_params(0, 2))     # an empty call is checked too


def test_with_and_without_timing(gpu_ctx, hand):
    res, exons, empty, q = hand
    want = UL.units(res, exons, empty, q, 9, 0)
    try:
        gpu_ctx.L.pgpu_set_timing(gpu_ctx.h, 0)
        same(device(gpu_ctx, res, exons, empty, q, 9, 0), want, "timing off")
        assert gpu_ctx.L.pgpu_unit_records_kernel_ms() == 0.0
    finally:
        gpu_ctx.L.pgpu_set_timing(gpu_ctx.h, 1)
    same(device(gpu_ctx, res, exons, empty, q, 9, 0), want, "timing on")
    assert gpu_ctx.L.pgpu_unit_records_kernel_ms() > 0.0


# ---- the plan form ----------------------------------------------------------------------------------------------------
def run_ladder(plan, prm=M.DEFAULTS):
    plan.run(prm["min_factor_len"], 0.2)
    plan.run_meg(**prm)
    plan.run_candidates(prm["min_factor_len"], prm["min_intron_length"])
    plan.run_factorizations(*F.DEFAULTS)
    plan.run_final_factorizations(40)


_product = {}


def product_records(source, retain, tmp_path_factory):
    """the records pintron_amd/bin/est-fact writes for the input, once per (input, setting) and process"""
    key = (source, retain)
    if key not in _product:
        gfa, efa = KL.real_inputs()[source]
        d = tmp_path_factory.mktemp("product_%s_%d" % key)
        _product[key] = UL.program_records(os.path.join(ROOT, "pintron_amd", "bin", "est-fact"), gfa, efa, retain, str(d))
    return _product[key]


@pytest.mark.parametrize("source,n_pat", [("c2", 307), ("issue13", 1891)])
@pytest.mark.parametrize("resident", [False, True])
def test_plan_form_against_the_restatement_the_plain_form_and_the_product(gpu_ctx, tmp_path_factory, source, n_pat, resident):
    import pintron_amd.capi as capi
    U = UL.real_units(source)
    seqs, genomic = U["working"], U["genomic"]
    assert len(seqs) == n_pat
    originals = {k: o for k, (w, o) in enumerate(zip(seqs, U["original"])) if o != w}
    assert originals
    q = UL.unit_queries(U)
    idx = capi.Index(gpu_ctx, genomic)
    plan = capi.PairingPlan(gpu_ctx, idx, seqs, resident=resident, originals=originals)
    try:
        run_ladder(plan)
        finals = plan.fetch_final_factorizations()
        res, exons, _ = finals
        empty = UL.empty_bits(plan.fetch_meg())
        assert empty.sum() > n_pat // 4
        for retain in (1, 0):
            n_bytes = plan.run_units(q, U["pref_N"], retain)
            got = plan.fetch_units()
            assert n_bytes == len(got[1]) == gpu_ctx.L.pgpu_pairing_plan_unit_bytes(plan.h) and plan.units_ms() > 0.0
            same(got, UL.units(res, exons, empty, q, U["pref_N"], retain), "the restatement on the device's own finals")
            same(got, device(gpu_ctx, res, exons, empty, q, U["pref_N"], retain), "the form without a plan")
            n_aligned, n_unaligned, wrong = UL.against_the_program(got[0], got[1], q, product_records(source, retain, tmp_path_factory))
            print("%s retain_externals %d: ALIGNED %d, UNALIGNED %d, HOST %d, disagreements with the product %d"
                  % (source, retain, n_aligned, n_unaligned, int((got[0]["verdict"] == 0).sum()), len(wrong)))
            assert not wrong, [(i, U["units"][i], got[0][i]) for i in wrong[:10]]
            assert n_aligned >= FLOORS[source][0] and n_unaligned >= FLOORS[source][1]
            # the finals are what they were, and a rerun gives the same bytes
            assert all(a.tobytes() == b.tobytes() for a, b in zip(plan.fetch_final_factorizations(), finals))
            assert plan.run_units(q, U["pref_N"], retain) == n_bytes
            same(plan.fetch_units(), got, "a rerun")
        # units in reverse, and a part of them: the blob follows the units
        back = q[::-1].copy()
        plan.run_units(back, U["pref_N"], 1)
        same(plan.fetch_units(), UL.units(res, exons, empty, back, U["pref_N"], 1), "in reverse")
        plan.run_units(q[5:40], 3, 0)
        same(plan.fetch_units(), UL.units(res, exons, empty, q[5:40], 3, 0), "a part")
        want = plan.fetch_units()
        # another plan run in between
        other = capi.PairingPlan(gpu_ctx, idx, seqs[:40], resident=resident)
        try:
            run_ladder(other)
            if resident:
                assert plan.fetch_units_raw(35)[0] == capi.PGPU_EINVAL and "overwritten" in message(gpu_ctx)
                assert plan.run_units_raw(q[5:40], 35, capi.unit_params(3, 0)) == capi.PGPU_EINVAL and "overwritten" in message(gpu_ctx)
                run_ladder(plan)
                plan.run_units(q[5:40], 3, 0)
            same(plan.fetch_units(), want, "after another plan")
        finally:
            other.close()
    finally:
        plan.close()
        idx.close()


def test_the_rules_of_the_sixth_rung(gpu_ctx):
    import pintron_amd.capi as capi
    L_ = gpu_ctx.L
    gfa, efa = M.rerun_input()
    exp, genomic = M.first_attempt_megs(gfa, efa)
    seqs = [e["seq"] for e in exp][:24]
    n_pat = len(seqs)
    idx = capi.Index(gpu_ctx, genomic)
    plan = capi.PairingPlan(gpu_ctx, idx, seqs)
    q = UL.query_array([(100 + k, 2 * k, 2 * k + 1, 0) for k in range(n_pat // 2)])
    prm = capi.unit_params(11, 1)

    def fetch_refused():
        return plan.fetch_units_raw(len(q), 1 << 16)[0] == capi.PGPU_EINVAL and "run_units first" in message(gpu_ctx)

    def run_refused(text, queries=q, n=None, params=prm):
        rc = plan.run_units_raw(queries, len(queries) if n is None else n, params)
        return rc == capi.PGPU_EINVAL and text in message(gpu_ctx) and L_.pgpu_pairing_plan_unit_bytes(plan.h) == 0 and plan.units_ms() == 0.0
    try:
        assert fetch_refused()                                                             # nothing ran yet
        assert run_refused("run_final_factorizations")
        plan.run(15, 0.2)
        plan.run_meg(**M.DEFAULTS)
        plan.run_candidates(15, 40)
        plan.run_factorizations(*F.DEFAULTS)
        assert run_refused("run_final_factorizations") and fetch_refused()
        plan.run_final_factorizations(40)
        finals = plan.fetch_final_factorizations()
        assert fetch_refused()
        # what the form without a plan refuses in q and params, null pointers, and the finals stay
        assert plan.run_units_raw(q, len(q), None) == capi.PGPU_EINVAL and plan.run_units_raw(None, len(q), prm) == capi.PGPU_EINVAL
        bad = q.copy()
        bad["fwd"][1] = n_pat
        assert run_refused("fwd is no pattern", bad)
        bad = q.copy()
        bad["rev"][1] = bad["fwd"][0]
        assert run_refused("named by two units", bad)
        assert run_refused("retain_externals above 1", params=capi.unit_params(0, 2))
        assert run_refused("more than 2^31 - 1", n=1 << 31)
        assert fetch_refused()
        assert all(a.tobytes() == b.tobytes() for a, b in zip(plan.fetch_final_factorizations(), finals))
        n_bytes = plan.run_units(q, 11, 1)
        want = plan.fetch_units()
        same(want, UL.units(finals[0], finals[1], UL.empty_bits(plan.fetch_meg()), q, 11, 1))
        assert plan.units_ms() > 0.0 and L_.pgpu_pairing_plan_unit_bytes(None) == 0 and L_.pgpu_pairing_plan_units_ms(None) == 0.0
        if n_bytes:
            assert plan.fetch_units_raw(len(q), n_bytes - 1)[0] == capi.PGPU_ENOSPC and message(gpu_ctx) == "blob too small"
        # no units at all: the rung is reached, nothing to fetch
        assert plan.run_units_raw(None, 0, prm) == capi.PGPU_OK and L_.pgpu_pairing_plan_unit_bytes(plan.h) == 0
        assert L_.pgpu_pairing_plan_fetch_units(gpu_ctx.h, plan.h, None, None, 0) == capi.PGPU_OK
        # a refused run lowers the plan to the finals, which stay
        plan.run_units(q, 11, 1)
        assert run_refused("flag bits", UL.query_array([(0, 0, 1, 4)])) and fetch_refused()
        assert all(a.tobytes() == b.tobytes() for a, b in zip(plan.fetch_final_factorizations(), finals))
        # a run of any earlier stage takes the units with it
        for rerun in (lambda: plan.run_final_factorizations(40), lambda: plan.run_factorizations(*F.DEFAULTS),
                      lambda: plan.run_candidates(15, 40), lambda: plan.run_meg(**M.DEFAULTS), lambda: plan.run(15, 0.2)):
            plan.run_units(q, 11, 1)
            rerun()
            assert fetch_refused()
            run_ladder(plan)
            assert plan.run_units(q, 11, 1) == n_bytes
            same(plan.fetch_units(), want, "after a rerun of an earlier stage")
    finally:
        plan.close()
    # an empty plan
    for resident in (False, True):
        empty = capi.PairingPlan(gpu_ctx, idx, [], resident=resident)
        try:
            assert empty.run_candidates(15, 40) == 0 and empty.run_factorizations(*F.DEFAULTS) == 0
            assert empty.run_final_factorizations(40) == 0
            assert empty.run_units_raw(None, 0, prm) == capi.PGPU_OK and empty.units_ms() == 0.0
            assert L_.pgpu_pairing_plan_fetch_units(gpu_ctx.h, empty.h, None, None, 0) == capi.PGPU_OK
            assert empty.run_units_raw(q[:1], 1, prm) == capi.PGPU_EINVAL and "fwd is no pattern" in message(gpu_ctx)
        finally:
            empty.close()
    idx.close()
