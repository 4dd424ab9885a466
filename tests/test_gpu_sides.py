"""GPU: the side stage (pgpu_unit_sides, pgpu_pairing_plan_run_sides) byte for byte against its restatement
(tests/side_lib.py) -- the form without a plan on the hand-made cases in one batch, in reverse and one by one, in batches
around the write pass's group of four waves and the count pass's group of 256, at the cap of 2^24 bytes, every refusal and
all three PGPU_ENOSPC shapes, with and without timing; the plan form on c2 and test-issue-13, plain and resident, against the
restatement on the device's own records, units and headers, against the form without a plan on the same arrays and against
the three files the product binary writes, per EST; the eighth rung's rules."""
import ctypes as C
import os

import numpy as np
import pytest

import cand_lib as KL
import fact_lib as F
import meg_lib as M
import side_lib as SL
import text_lib as TL
import unit_lib as UL

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("megs", "pmegs", "edges")


def message(ctx):
    return ctx.L.pgpu_last_error(ctx.h).decode()


def device(ctx, q, units, records, headers, seqs):
    import pintron_amd.capi as capi
    return capi.unit_sides(ctx, q, units, records, headers, seqs)


def same(got, want, what=""):
    assert got[0].dtype == want[0].dtype and len(got[0]) == len(want[0]), what
    for f in got[0].dtype.names if len(got[0]) else ():
        bad = np.nonzero((got[0][f] != want[0][f]).reshape(len(got[0]), -1).any(axis=1))[0]
        assert len(bad) == 0, (what, f, int(bad[0]), got[0][int(bad[0])], want[0][int(bad[0])])
    for k, name in enumerate(NAMES, 1):
        if got[k] != want[k]:
            a, b = np.frombuffer(got[k], dtype=np.uint8), np.frombuffer(want[k], dtype=np.uint8)
            n = min(len(a), len(b))
            at = int(np.nonzero(a[:n] != b[:n])[0][0]) if (a[:n] != b[:n]).any() else n
            raise AssertionError((what, name, len(a), len(b), at, got[k][max(0, at - 40):at + 40], want[k][max(0, at - 40):at + 40]))


@pytest.fixture(scope="module")
def hand():
    batch = SL.batch(SL.hand_cases())
    return batch, SL.sides(*batch)


def test_hand_made_cases_in_one_batch_in_reverse_and_one_by_one(gpu_ctx, hand):
    import pintron_amd.capi as capi
    (q, units, records, headers, seqs), want = hand
    same(device(gpu_ctx, q, units, records, headers, seqs), want, "one batch")
    assert gpu_ctx.L.pgpu_unit_sides_kernel_ms() > 0.0
    assert {int(v) for v in want[0]["verdict"]} == {SL.NONE, SL.DONE, SL.HOST}
    qb, ub, hb = q[::-1].copy(), units[::-1].copy(), headers[::-1]
    same(device(gpu_ctx, qb, ub, records, hb, seqs), SL.sides(qb, ub, records, hb, seqs), "in reverse")
    rb, rf = capi._offsets(records)
    sb, sf = capi._offsets(seqs)
    for i in range(len(units)):
        lens = tuple(int(want[0][f + "_bytes"][i]) for f in NAMES)
        hb1, hf1 = capi._offsets(headers[i:i + 1])
        rc, out, blobs, got_lens = capi.unit_sides_raw(gpu_ctx, q[i:i + 1], units[i:i + 1], 1, rb, rf, len(records), hb1, hf1, sb, sf, lens)
        assert rc == capi.PGPU_OK and got_lens == lens, (i, rc, got_lens, lens)
        for k, f in enumerate(NAMES):
            a = int(want[0][f + "_first"][i])
            assert blobs[k].tobytes() == want[1 + k][a:a + lens[k]], (i, f)
        one = want[0][i:i + 1].copy()
        for f in NAMES:
            one[f + "_first"] = 0
        assert out.tobytes() == one.tobytes(), (i, out, one)


@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 255, 256, 257])
def test_batches_around_the_groups_of_the_two_passes(gpu_ctx, n):
    cases = SL.hand_cases()
    picked = [cases[(37 * k) % len(cases)] for k in range(max(n, 1))]
    q, units, records, headers, seqs = SL.batch(picked, seed=n)
    q, units, headers = q[:n], units[:n], headers[:n]
    same(device(gpu_ctx, q, units, records, headers, seqs), SL.sides(q, units, records, headers, seqs), n)


def test_the_cap_on_a_units_bytes(gpu_ctx):
    cap = SL.cap_cases()
    batch = SL.batch(cap)
    want = SL.sides(*batch)
    got = device(gpu_ctx, *batch)
    same(got, want)
    by = {c["name"]: got[0][i] for i, c in enumerate(cap)}
    assert (int(by["cap_exact"]["verdict"]), int(by["cap_exact"]["megs_bytes"])) == (SL.DONE, SL.MAX_UNIT_BYTES)
    assert int(by["cap_one_over"]["verdict"]) == SL.HOST and int(by["cap_pmegs_alone"]["verdict"]) == SL.HOST
    assert int(by["cap_pmegs_exact_megs_over"]["verdict"]) == SL.HOST
    assert (int(by["cap_megs_exact"]["verdict"]), int(by["cap_megs_exact"]["megs_bytes"]), int(by["cap_megs_exact"]["pmegs_bytes"])) == \
        (SL.DONE, SL.MAX_UNIT_BYTES, SL.MAX_UNIT_BYTES - 15)


def test_every_refusal_and_all_three_enospc_shapes(gpu_ctx, hand):
    import pintron_amd.capi as capi
    (q, units, records, headers, seqs), want = hand
    n, n_pat = len(units), len(seqs)
    rb, rf = capi._offsets(records)
    hb, hf = capi._offsets(headers)
    sb, sf = capi._offsets(seqs)
    totals = tuple(len(want[k]) for k in (1, 2, 3))

    def call(q=q, units=units, n=n, rb=rb, rf=rf, n_pat=n_pat, hb=hb, hf=hf, sb=sb, sf=sf, caps=totals, **kw):
        rc, out, blobs, lens = capi.unit_sides_raw(gpu_ctx, q, units, n, rb, rf, n_pat, hb, hf, sb, sf, caps, **kw)
        if rc != capi.PGPU_OK:
            assert not out.view(np.uint8).any() and not any(b.any() for b in blobs)     # nothing written
            assert gpu_ctx.L.pgpu_unit_sides_kernel_ms() == 0.0
        return rc, lens

    assert call() == (capi.PGPU_OK, totals)

    def refused(text, **kw):
        rc = call(**kw)[0]
        return rc == capi.PGPU_EINVAL and text in message(gpu_ctx)

    def changed(arr, i, value, field=None):
        a = arr.copy()
        if field is None:
            a[i] = value
        else:
            a[field][i] = value
        return a
    by = {c["name"]: i for i, c in enumerate(SL.hand_cases())}
    rev_unit, fwd_unit, host_unit = by["aligned_rev"], by["aligned_fwd_with_sibling"], by["host_between"]
    lone, un_rev, flagged_host = by["aligned_fwd_no_sibling"], by["unaligned_rev"], by["host_over_flagged"]
    assert refused("bad record offsets", rf=changed(rf, 3, int(rf[4]) + 4))
    assert refused("bad record offsets", rf=changed(rf, n_pat, len(rb) + 4))
    assert refused("bad record offsets", recs_len=len(rb) - 4)
    assert refused("bad record offsets", rf=changed(rf, 5, int(rf[5]) + 2))
    assert refused("bad header offsets", hf=changed(hf, 3, int(hf[4]) + 1))
    assert refused("bad header offsets", hf=changed(hf, n, len(hb) + 1))
    assert refused("bad header offsets", headers_len=len(hb) - 1)
    assert refused("bad sequence offsets", sf=changed(sf, 7, int(sf[8]) + 1))
    assert refused("bad sequence offsets", sf=changed(sf, n_pat, len(sb) + 1))
    assert refused("bad sequence offsets", seqs_len=len(sb) - 1)
    assert refused("a verdict above 2", units=changed(units, 2, 3, "verdict"))
    assert refused("a verdict above 2", units=changed(units, host_unit, 255, "verdict"))
    assert refused("a strand above 1", units=changed(units, rev_unit, 2, "strand"))
    assert refused("fwd is no pattern", q=changed(q, lone, n_pat, "fwd"))
    assert refused("rev is neither a pattern", q=changed(q, rev_unit, n_pat, "rev"))
    assert refused("rev is neither a pattern", q=changed(q, host_unit, 0xfffffffe, "rev"))
    assert refused("strand 1 without a sibling", units=changed(units, lone, 1, "strand"))
    assert refused("not the query's pattern", units=changed(units, rev_unit, int(q["fwd"][rev_unit]), "pattern"))
    assert refused("not the query's pattern", units=changed(units, fwd_unit, int(q["rev"][fwd_unit]), "pattern"))
    assert refused("not the query's pattern", units=changed(units, host_unit, n_pat, "pattern"))
    # a settled unit over a flagged record: the HOST unit that names two of them, settled
    assert refused("flagged record", units=changed(units, flagged_host, UL.U_UNALIGNED, "verdict"))
    assert refused("flagged record", units=changed(changed(changed(units, flagged_host, UL.U_ALIGNED, "verdict"), flagged_host, 1, "strand"),
                                                   flagged_host, int(q["rev"][flagged_host]), "pattern"),
                   q=changed(q, flagged_host, int(q["fwd"][lone]), "fwd"))                  # the sibling alone is flagged
    flag_at = int(rf[int(q["fwd"][un_rev])]) + 8
    assert refused("flagged record", rb=rb[:flag_at] + b"\1" + rb[flag_at + 1:])
    # ... and over a record that does not add up: its lengths say more than the record holds
    p = int(q["rev"][rev_unit])
    nv, ne = np.frombuffer(rb, dtype="<u4", count=2, offset=int(rf[p]))
    lens_at = int(rf[p]) + ((16 + 12 * int(nv) + 2 * (int(nv) + 1) + int(ne) + 3) & ~3)
    ml, xl = (int(v) for v in np.frombuffer(rb, dtype="<u4", count=2, offset=lens_at))
    room = int(rf[p + 1]) - lens_at - 8
    for new_ml, new_xl in ((ml, room - ml + 1), (room + 1, 0), (0xfffffff0, 0x20)):
        broken = rb[:lens_at] + np.array([new_ml, new_xl], dtype="<u4").tobytes() + rb[lens_at + 8:]
        assert refused("pass the next record", rb=broken), (new_ml, new_xl)
    broken = rb[:int(rf[p])] + np.array([0xffffffff], dtype="<u4").tobytes() + rb[int(rf[p]) + 4:]
    assert refused("pass the next record", rb=broken)
    assert refused("more than 2^31 - 1", n=1 << 31)                                         # counts alone: no unit is read
    assert refused("more than 2^31 - 1", n_pat=1 << 31, n=0, q=q[:0], units=units[:0], hf=hf[:1])
    # a HOST unit's records are not looked at
    assert call(rb=rb[:int(rf[int(q["fwd"][host_unit])])] + b"\xff" * 16 + rb[int(rf[int(q["fwd"][host_unit])]) + 16:])[0] == capi.PGPU_OK
    # null pointers: a bare PGPU_EINVAL
    L_ = gpu_ctx.L
    out = np.zeros(n, dtype=np.dtype(capi.SIDE_RESULT_DTYPE))
    blobs = [np.zeros(t, dtype=np.uint8) for t in totals]
    lens = (C.c_size_t * 3)()
    v = lambda x: C.cast(C.c_char_p(x), C.c_void_p)
    u64p = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64))
    args = [gpu_ctx.h, q.ctypes.data_as(C.POINTER(capi.UnitQuery)), units.ctypes.data_as(C.POINTER(capi.UnitResult)), n,
            v(rb), len(rb), u64p(rf), n_pat, v(hb), len(hb), u64p(hf), v(sb), len(sb), u64p(sf),
            out.ctypes.data_as(C.POINTER(capi.SideResult)), blobs[0].ctypes.data_as(C.c_void_p), totals[0],
            blobs[1].ctypes.data_as(C.c_void_p), totals[1], blobs[2].ctypes.data_as(C.c_void_p), totals[2], lens]
    assert L_.pgpu_unit_sides(*args) == capi.PGPU_OK and all(blobs[k].tobytes() == want[1 + k] for k in range(3))
    for at in (0, 1, 2, 4, 6, 8, 10, 11, 13, 14, 15, 17, 19, 21):
        a = list(args)
        a[at] = None
        assert L_.pgpu_unit_sides(*a) == capi.PGPU_EINVAL, at
    # PGPU_ENOSPC with the three needed sizes, nothing written: each cap too small, and all
    for caps in ((totals[0] - 1, totals[1], totals[2]), (totals[0], totals[1] - 1, totals[2]), (totals[0], totals[1], totals[2] - 1),
                 (0, 0, 0)):
        rc, got = call(caps=caps)
        assert rc == capi.PGPU_ENOSPC and got == totals and message(gpu_ctx) == "side buffers too small"
    assert call(q=q[:0], units=units[:0], n=0, hf=hf[:1]) == (capi.PGPU_OK, (0, 0, 0))
    assert call(q=q[:0], units=units[:0], n=0, hf=hf[:1], caps=(0, 0, 0)) == (capi.PGPU_OK, (0, 0, 0))
    assert refused("bad sequence offsets", q=q[:0], units=units[:0], n=0, hf=hf[:1], seqs_len=3)    # an empty call is checked too


def test_with_and_without_timing(gpu_ctx, hand):
    batch, want = hand
    try:
        gpu_ctx.L.pgpu_set_timing(gpu_ctx.h, 0)
        same(device(gpu_ctx, *batch), want, "timing off")
        assert gpu_ctx.L.pgpu_unit_sides_kernel_ms() == 0.0
    finally:
        gpu_ctx.L.pgpu_set_timing(gpu_ctx.h, 1)
    same(device(gpu_ctx, *batch), want, "timing on")
    assert gpu_ctx.L.pgpu_unit_sides_kernel_ms() > 0.0


# ---- the plan form, and the product's own files -----------------------------------------------------------------------
_product = {}


def product_sides(source, tmp_path_factory):
    """the three side files pintron_amd/bin/est-fact writes for the input, cut per EST; once per input and process"""
    if source not in _product:
        gfa, efa = KL.real_inputs()[source]
        d = str(tmp_path_factory.mktemp("product_sides_" + source))
        UL.program_records(os.path.join(ROOT, "pintron_amd", "bin", "est-fact"), gfa, efa, 1, d)
        _product[source] = SL.per_est(TL.est_headers(efa), *SL.program_sides(d))
    return _product[source]


def run_ladder(plan, prm=M.DEFAULTS):
    plan.run(prm["min_factor_len"], 0.2)
    plan.run_meg(**prm)
    plan.run_candidates(prm["min_factor_len"], prm["min_intron_length"])
    plan.run_factorizations(*F.DEFAULTS)
    plan.run_final_factorizations(40)


@pytest.mark.parametrize("source,n_pat", [("c2", 307), ("issue13", 1891)])
@pytest.mark.parametrize("resident", [False, True])
def test_plan_form_against_the_restatement_the_plain_form_and_the_product(gpu_ctx, tmp_path_factory, source, n_pat, resident):
    import pintron_amd.capi as capi
    U = UL.real_units(source)
    gfa, efa = KL.real_inputs()[source]
    seqs, genomic = U["working"], U["genomic"]
    assert len(seqs) == n_pat
    originals = {k: o for k, (w, o) in enumerate(zip(seqs, U["original"])) if o != w}
    assert originals
    q = UL.unit_queries(U)
    ids = TL.est_headers(efa)
    headers = [ids[int(i)] for i in q["est_index"]]
    theirs = product_sides(source, tmp_path_factory)
    idx = capi.Index(gpu_ctx, genomic)
    src = capi.TextSource(gpu_ctx, TL.original_genomic(gfa))
    plan = capi.PairingPlan(gpu_ctx, idx, seqs, resident=resident, originals=originals)
    try:
        run_ladder(plan)
        records = plan.fetch_meg()
        plan.run_units(q, U["pref_N"], 1)
        units, blob = plan.fetch_units()
        plan.run_texts(src, headers)
        texts = plan.fetch_texts()
        for again in range(2):
            sizes = plan.run_sides()
            got = plan.fetch_sides()
            assert sizes == tuple(len(b) for b in got[1:]) and plan.sides_ms() >= plan.sides_write_ms() > 0.0
            same(got, SL.sides(q, units, records, headers, U["original"]), "the restatement on the device's own records and units")
            same(got, device(gpu_ctx, q, units, records, headers, U["original"]), "the form without a plan")
            # each DONE unit against that EST's texts in the product's files
            n_done = n_rev = n_un = 0
            for i in np.nonzero(got[0]["verdict"] == SL.DONE)[0]:
                mine = tuple(got[1 + k][int(got[0][f + "_first"][i]):int(got[0][f + "_first"][i]) + int(got[0][f + "_bytes"][i])]
                             for k, f in enumerate(NAMES))
                assert theirs[int(q["est_index"][i])] == mine, (i, U["units"][i])
                n_done += 1
                n_rev += int(units["verdict"][i]) == UL.U_ALIGNED and int(units["strand"][i]) == 1
                n_un += int(units["verdict"][i]) == UL.U_UNALIGNED and int(units["strand"][i]) == 1
            n_aligned = int((units["verdict"] == UL.U_ALIGNED).sum())
            assert n_done == int((units["verdict"] != UL.U_HOST).sum()) and n_aligned >= (140 if source == "c2" else 750) and n_un >= 1
            assert source == "c2" or n_rev >= 1
            print("%s: %d DONE units (%d ALIGNED, %d on the sibling, %d UNALIGNED with a sibling), megs %d, pmegs %d, edges %d bytes"
                  % ((source, n_done, n_aligned, n_rev, n_un) + sizes))
            # texts, units and finals are what they were behind the sides
            t2, u2 = plan.fetch_texts(), plan.fetch_units()
            assert t2[0].tobytes() == texts[0].tobytes() and t2[1:] == texts[1:] and u2[0].tobytes() == units.tobytes() and u2[1] == blob
        # units in reverse: the sides follow the units
        back, hback = q[::-1].copy(), headers[::-1]
        plan.run_units(back, U["pref_N"], 1)
        units = plan.fetch_units()[0]
        plan.run_texts(src, hback)
        plan.run_sides()
        want = plan.fetch_sides()
        same(want, SL.sides(back, units, records, hback, U["original"]), "in reverse")
        # a plan without originals prints the working sequences
        bare = capi.PairingPlan(gpu_ctx, idx, seqs, resident=resident)
        try:
            run_ladder(bare)
            bare.run_units(back, U["pref_N"], 1)
            u2 = bare.fetch_units()[0]
            bare.run_texts(src, hback)
            bare.run_sides()
            got2 = bare.fetch_sides()
            same(got2, SL.sides(back, u2, bare.fetch_meg(), hback, seqs), "without originals")
            assert got2[1] != want[1]
            if resident:                                    # `bare` ran in between: nothing of `plan` is left
                assert plan.fetch_sides_raw(len(q))[0] == capi.PGPU_EINVAL and "overwritten" in message(gpu_ctx)
                assert plan.run_sides_raw() == capi.PGPU_EINVAL and "overwritten" in message(gpu_ctx)
                run_ladder(plan)
                plan.run_units(back, U["pref_N"], 1)
                plan.run_texts(src, hback)
                plan.run_sides()
            same(plan.fetch_sides(), want, "after another plan")
        finally:
            bare.close()
    finally:
        plan.close()
        src.close()
        idx.close()


def test_the_rules_of_the_eighth_rung(gpu_ctx):
    import pintron_amd.capi as capi
    L_ = gpu_ctx.L
    gfa, efa = M.rerun_input()
    exp, genomic = M.first_attempt_megs(gfa, efa)
    seqs = [e["seq"] for e in exp][:24]
    n_pat = len(seqs)
    idx = capi.Index(gpu_ctx, genomic)
    src = capi.TextSource(gpu_ctx, genomic)
    plan = capi.PairingPlan(gpu_ctx, idx, seqs)
    q = UL.query_array([(100 + k, 2 * k, 2 * k + 1, 0) for k in range(n_pat // 2)])
    headers = [b"/gb=R%03d" % k + b"x" * (k % 5) for k in range(len(q))]
    big = (1 << 20,) * 3

    def fetch_refused():
        return plan.fetch_sides_raw(len(q), big)[0] == capi.PGPU_EINVAL and "run_sides first" in message(gpu_ctx)

    def run_refused(text):
        rc = plan.run_sides_raw()
        return (rc == capi.PGPU_EINVAL and text in message(gpu_ctx) and all(plan.side_bytes(k) == 0 for k in range(3)) and
                plan.sides_ms() == 0.0 and plan.sides_write_ms() == 0.0)
    try:
        assert fetch_refused() and run_refused("run_texts")                                 # nothing ran yet
        run_ladder(plan)
        assert fetch_refused() and run_refused("run_texts")
        plan.run_units(q, 11, 1)
        units = plan.fetch_units()
        finals = plan.fetch_final_factorizations()
        records = plan.fetch_meg()
        assert fetch_refused() and run_refused("run_texts")                                 # run_sides before run_texts
        assert plan.fetch_units()[1] == units[1]
        plan.run_texts(src, headers)
        texts = plan.fetch_texts()
        assert fetch_refused()                                                              # a fetch before the run
        assert L_.pgpu_pairing_plan_run_sides(None, plan.h) == capi.PGPU_EINVAL and L_.pgpu_pairing_plan_run_sides(gpu_ctx.h, None) == capi.PGPU_EINVAL
        sizes = plan.run_sides()
        want = plan.fetch_sides()
        same(want, SL.sides(q, units[0], records, headers, seqs))
        assert (want[0]["verdict"] == SL.DONE).any()
        assert plan.sides_ms() >= plan.sides_write_ms() > 0.0
        assert L_.pgpu_pairing_plan_side_bytes(None, 0) == 0 and L_.pgpu_pairing_plan_sides_ms(None) == 0.0
        assert L_.pgpu_pairing_plan_sides_write_ms(None) == 0.0 and plan.side_bytes(3) == 0 and plan.side_bytes(-1) == 0
        for k in range(3):
            if sizes[k]:
                caps = list(sizes)
                caps[k] -= 1
                assert plan.fetch_sides_raw(len(q), caps)[0] == capi.PGPU_ENOSPC and message(gpu_ctx) == "side buffers too small"
        assert L_.pgpu_pairing_plan_fetch_sides(gpu_ctx.h, plan.h, None, None, 0, None, 0, None, 0) == capi.PGPU_EINVAL
        # texts, units and finals are unchanged behind the sides; a rerun gives the same bytes
        t2, u2 = plan.fetch_texts(), plan.fetch_units()
        assert t2[0].tobytes() == texts[0].tobytes() and t2[1:] == texts[1:] and u2[0].tobytes() == units[0].tobytes() and u2[1] == units[1]
        assert all(a.tobytes() == b.tobytes() for a, b in zip(plan.fetch_final_factorizations(), finals))
        assert plan.run_sides() == sizes
        same(plan.fetch_sides(), want, "a rerun")
        # a run of any earlier stage, run_texts included, takes the sides with it
        for rerun in (lambda: plan.run_texts(src, headers), lambda: plan.run_units(q, 11, 1), lambda: plan.run_final_factorizations(40),
                      lambda: plan.run_factorizations(*F.DEFAULTS), lambda: plan.run_candidates(15, 40),
                      lambda: plan.run_meg(**M.DEFAULTS), lambda: plan.run(15, 0.2)):
            plan.run_sides()
            rerun()
            assert fetch_refused()
            run_ladder(plan)
            plan.run_units(q, 11, 1)
            plan.run_texts(src, headers)
            assert plan.run_sides() == sizes
            same(plan.fetch_sides(), want, "after a rerun of an earlier stage")
        # without timing: the same bytes, no milliseconds
        try:
            L_.pgpu_set_timing(gpu_ctx.h, 0)
            assert plan.run_sides() == sizes
            same(plan.fetch_sides(), want, "timing off")
        finally:
            L_.pgpu_set_timing(gpu_ctx.h, 1)
        # a run of zero units: the rung is reached, nothing to fetch
        assert plan.run_units_raw(None, 0, capi.unit_params(11, 1)) == capi.PGPU_OK
        assert plan.run_texts_raw(src, None, 0, None) == capi.PGPU_OK
        assert plan.run_sides_raw() == capi.PGPU_OK and all(plan.side_bytes(k) == 0 for k in range(3))
        assert L_.pgpu_pairing_plan_fetch_sides(gpu_ctx.h, plan.h, None, None, 0, None, 0, None, 0) == capi.PGPU_OK
    finally:
        plan.close()
    # a plan made without timing has no events: 0 milliseconds
    try:
        L_.pgpu_set_timing(gpu_ctx.h, 0)
        quiet = capi.PairingPlan(gpu_ctx, idx, seqs)
        try:
            run_ladder(quiet)
            quiet.run_units(q, 11, 1)
            quiet.run_texts(src, headers)
            assert quiet.run_sides() == sizes
            same(quiet.fetch_sides(), want, "a plan without timing")
            assert quiet.sides_ms() == 0.0 and quiet.sides_write_ms() == 0.0
        finally:
            quiet.close()
    finally:
        L_.pgpu_set_timing(gpu_ctx.h, 1)
    # an empty plan
    for resident in (False, True):
        empty = capi.PairingPlan(gpu_ctx, idx, [], resident=resident)
        try:
            assert empty.run_sides_raw() == capi.PGPU_EINVAL and "run_texts" in message(gpu_ctx)
            assert empty.run_candidates(15, 40) == 0 and empty.run_factorizations(*F.DEFAULTS) == 0
            assert empty.run_final_factorizations(40) == 0
            assert empty.run_units_raw(None, 0, capi.unit_params(11, 1)) == capi.PGPU_OK
            assert empty.run_texts_raw(src, None, 0, None) == capi.PGPU_OK
            assert empty.run_sides_raw() == capi.PGPU_OK and empty.sides_ms() == 0.0
            assert L_.pgpu_pairing_plan_fetch_sides(gpu_ctx.h, empty.h, None, None, 0, None, 0, None, 0) == capi.PGPU_OK
        finally:
            empty.close()
    src.close()
    idx.close()
