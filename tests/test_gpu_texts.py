"""GPU: the text stage (pgpu_unit_texts, pgpu_pairing_plan_run_texts) byte for byte against its restatement
(tests/text_lib.py) -- the form without a plan on the hand-made cases in one batch, in reverse and one by one, in batches
around the write pass's group of four waves and the count pass's group of 256, at the cap of 2^24 bytes, every refusal and
both PGPU_ENOSPC shapes, with and without timing; the records the product binary writes for c2 and test-issue-13 against its
own two files, whole; the plan form on the same inputs, plain and resident, against the restatement on the device's own
units, against the form without a plan on the same arrays and against the product's files per EST; the seventh rung's rules."""
import ctypes as C
import os

import numpy as np
import pytest

import cand_lib as KL
import fact_lib as F
import meg_lib as M
import text_lib as TL
import unit_lib as UL

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def message(ctx):
    return ctx.L.pgpu_last_error(ctx.h).decode()


def device(ctx, units, blob, headers, seqs, genomic):
    import pintron_amd.capi as capi
    return capi.unit_texts(ctx, units, blob, headers, seqs, genomic)


def same(got, want, what=""):
    assert got[0].dtype == want[0].dtype and len(got[0]) == len(want[0]), what
    for f in got[0].dtype.names if len(got[0]) else ():
        bad = np.nonzero((got[0][f] != want[0][f]).reshape(len(got[0]), -1).any(axis=1))[0]
        assert len(bad) == 0, (what, f, int(bad[0]), got[0][int(bad[0])], want[0][int(bad[0])])
    for k, name in ((1, "raw"), (2, "pests")):
        if got[k] != want[k]:
            a, b = np.frombuffer(got[k], dtype=np.uint8), np.frombuffer(want[k], dtype=np.uint8)
            n = min(len(a), len(b))
            at = int(np.nonzero(a[:n] != b[:n])[0][0]) if (a[:n] != b[:n]).any() else n
            raise AssertionError((what, name, len(a), len(b), at, got[k][max(0, at - 40):at + 40], want[k][max(0, at - 40):at + 40]))


@pytest.fixture(scope="module")
def hand():
    batch = TL.batch(TL.hand_cases())
    return batch, TL.texts(*batch, TL.genomic())


def test_hand_made_cases_in_one_batch_in_reverse_and_one_by_one(gpu_ctx, hand):
    import pintron_amd.capi as capi
    (units, blob, headers, seqs), want = hand
    G = TL.genomic()
    same(device(gpu_ctx, units, blob, headers, seqs, G), want, "one batch")
    assert gpu_ctx.L.pgpu_unit_texts_kernel_ms() > 0.0
    back, hback = units[::-1].copy(), headers[::-1]
    same(device(gpu_ctx, back, blob, hback, seqs, G), TL.texts(back, blob, hback, seqs, G), "in reverse")
    sb, sf = capi._offsets(seqs)
    for i in range(len(units)):
        a, n, b, m = (int(want[0][f][i]) for f in ("raw_first", "raw_bytes", "pests_first", "pests_bytes"))
        hb, hf = capi._offsets(headers[i:i + 1])
        rc, out, raw, pests, rl, pl = capi.unit_texts_raw(gpu_ctx, units[i:i + 1], 1, blob, hb, hf, sb, sf, len(seqs), G, n, m)
        assert rc == capi.PGPU_OK and (rl, pl) == (n, m), (i, rc, rl, pl)
        assert raw.tobytes() == want[1][a:a + n] and pests.tobytes() == want[2][b:b + m], i
        one = want[0][i:i + 1].copy()
        one["raw_first"] = one["pests_first"] = 0
        assert out.tobytes() == one.tobytes(), (i, out, one)


@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 255, 256, 257])
def test_batches_around_the_groups_of_the_two_passes(gpu_ctx, n):
    cases = TL.hand_cases()
    picked = [cases[(37 * k) % len(cases)] for k in range(max(n, 1))]
    units, blob, headers, seqs = TL.batch(picked, seed=n)
    units, headers = units[:n], headers[:n]
    same(device(gpu_ctx, units, blob, headers, seqs, TL.genomic()), TL.texts(units, blob, headers, seqs, TL.genomic()), n)


def test_the_cap_on_a_units_bytes(gpu_ctx):
    cap = TL.cap_cases()
    batch = TL.batch(cap)
    want = TL.texts(*batch, TL.genomic())
    got = device(gpu_ctx, *batch, TL.genomic())
    same(got, want)
    by = {c["name"]: got[0][i] for i, c in enumerate(cap)}
    assert (int(by["cap_exact"]["verdict"]), int(by["cap_exact"]["raw_bytes"])) == (TL.DONE, TL.MAX_UNIT_BYTES)
    assert int(by["cap_one_over"]["verdict"]) == TL.HOST and int(by["cap_pests_alone"]["verdict"]) == TL.HOST
    assert (int(by["cap_pests_exact"]["verdict"]), int(by["cap_pests_exact"]["pests_bytes"])) == (TL.DONE, TL.MAX_UNIT_BYTES)


def test_every_refusal_and_both_enospc_shapes(gpu_ctx, hand):
    import pintron_amd.capi as capi
    (units, blob, headers, seqs), want = hand
    G = TL.genomic()
    n, n_pat = len(units), len(seqs)
    hb, hf = capi._offsets(headers)
    sb, sf = capi._offsets(seqs)
    raw_total, pests_total = len(want[1]), len(want[2])

    def call(units=units, n=n, blob=blob, hb=hb, hf=hf, sb=sb, sf=sf, n_pat=n_pat, raw_cap=raw_total, pests_cap=pests_total, **kw):
        rc, out, raw, pests, rl, pl = capi.unit_texts_raw(gpu_ctx, units, n, blob, hb, hf, sb, sf, n_pat, G, raw_cap, pests_cap, **kw)
        if rc != capi.PGPU_OK:
            assert not out.view(np.uint8).any() and not raw.any() and not pests.any()     # nothing written
            assert gpu_ctx.L.pgpu_unit_texts_kernel_ms() == 0.0
        return rc, rl, pl

    assert call() == (capi.PGPU_OK, raw_total, pests_total)

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
    aligned = np.nonzero(units["verdict"] == UL.U_ALIGNED)[0]
    big = int(aligned[np.argmax(units["n_bytes"][aligned])])
    last = int(aligned[np.argmax(units["first_byte"][aligned])])
    k = int(aligned[5])
    assert refused("bad header offsets", hf=changed(hf, 3, int(hf[4]) + 1))
    assert refused("bad header offsets", hf=changed(hf, n, len(hb) + 1))
    assert refused("bad header offsets", headers_len=len(hb) - 1)
    assert refused("bad sequence offsets", sf=changed(sf, 7, int(sf[8]) + 1))
    assert refused("bad sequence offsets", sf=changed(sf, n_pat, len(sb) + 1))
    assert refused("bad sequence offsets", seqs_len=len(sb) - 1)
    assert refused("a verdict above 2", units=changed(units, 2, 3, "verdict"))
    assert refused("a verdict above 2", units=changed(units, 2, 255, "verdict"))
    assert refused("pattern is no pattern", units=changed(units, k, n_pat, "pattern"))
    assert refused("pattern is no pattern", n_pat=int(units["pattern"][aligned].max()), sf=sf[:int(units["pattern"][aligned].max()) + 1])
    assert refused("beyond the blob", units=changed(units, last, int(units["first_byte"][last]) + 4, "first_byte"))
    assert refused("beyond the blob", units=changed(units, k, 1 << 40, "first_byte"))
    assert refused("beyond the blob", blob_len=len(blob) - 4)
    assert refused("no multiple of 4", units=changed(units, k, int(units["first_byte"][k]) + 2, "first_byte"))
    assert refused("no multiple of 4", units=changed(units, k, int(units["n_bytes"][k]) + 1, "n_bytes"))
    assert refused("do not add up", units=changed(units, big, int(units["n_bytes"][big]) - 16, "n_bytes"))
    assert refused("do not add up", units=changed(units, big, int(units["n_bytes"][big]) - 4, "n_bytes"))
    broken = bytearray(blob)
    broken[int(units["first_byte"][big]) + 4] += 1                                          # one factorization more than there is
    assert refused("do not add up", blob=bytes(broken))
    assert refused("shorter than its 8 bytes", units=changed(units, k, 4, "n_bytes"))
    assert refused("more than 2^31 - 1", n=1 << 31)                                         # counts alone: no unit is read
    assert refused("more than 2^31 - 1", n_pat=1 << 31, n=0, units=units[:0], hf=hf[:1])
    # a unit that is not ALIGNED is not looked at beyond its verdict
    idle = int(np.nonzero(units["verdict"] != UL.U_ALIGNED)[0][0])
    assert call(units=changed(units, idle, 0xffffffff, "pattern"))[0] == capi.PGPU_OK
    # null pointers: a bare PGPU_EINVAL
    L_ = gpu_ctx.L
    out = np.zeros(n, dtype=np.dtype(capi.TEXT_RESULT_DTYPE))
    raw, pests = np.zeros(raw_total, dtype=np.uint8), np.zeros(pests_total, dtype=np.uint8)
    rl, pl = C.c_size_t(0), C.c_size_t(0)
    v = lambda x: C.cast(C.c_char_p(x), C.c_void_p)
    args = [gpu_ctx.h, units.ctypes.data_as(C.POINTER(capi.UnitResult)), n, v(blob), len(blob), v(hb), len(hb),
            hf.ctypes.data_as(C.POINTER(C.c_uint64)), v(sb), len(sb), sf.ctypes.data_as(C.POINTER(C.c_uint64)), n_pat, v(G), len(G),
            out.ctypes.data_as(C.POINTER(capi.TextResult)), raw.ctypes.data_as(C.c_void_p), raw_total, C.byref(rl),
            pests.ctypes.data_as(C.c_void_p), pests_total, C.byref(pl)]
    assert L_.pgpu_unit_texts(*args) == capi.PGPU_OK and raw.tobytes() == want[1]
    for at in (0, 1, 3, 5, 7, 8, 10, 12, 14, 15, 17, 18, 20):
        a = list(args)
        a[at] = None
        assert L_.pgpu_unit_texts(*a) == capi.PGPU_EINVAL, at
    # PGPU_ENOSPC with both needed sizes, nothing written: raw too small, pests too small, both
    for raw_cap, pests_cap in ((raw_total - 1, pests_total), (raw_total, pests_total - 1), (0, 0), (raw_total - 1, 0)):
        rc, a, b = call(raw_cap=raw_cap, pests_cap=pests_cap)
        assert rc == capi.PGPU_ENOSPC and (a, b) == (raw_total, pests_total) and message(gpu_ctx) == "text buffers too small"
    assert call(units=units[:0], n=0, hf=hf[:1]) == (capi.PGPU_OK, 0, 0)
    assert call(units=units[:0], n=0, hf=hf[:1], raw_cap=0, pests_cap=0) == (capi.PGPU_OK, 0, 0)
    assert refused("bad sequence offsets", units=units[:0], n=0, hf=hf[:1], seqs_len=3)    # an empty call is checked too


def test_with_and_without_timing(gpu_ctx, hand):
    batch, want = hand
    try:
        gpu_ctx.L.pgpu_set_timing(gpu_ctx.h, 0)
        same(device(gpu_ctx, *batch, TL.genomic()), want, "timing off")
        assert gpu_ctx.L.pgpu_unit_texts_kernel_ms() == 0.0
    finally:
        gpu_ctx.L.pgpu_set_timing(gpu_ctx.h, 1)
    same(device(gpu_ctx, *batch, TL.genomic()), want, "timing on")
    assert gpu_ctx.L.pgpu_unit_texts_kernel_ms() > 0.0


# ---- the product's own records and files -----------------------------------------------------------------------------
_product = {}


def product_texts(source, retain, tmp_path_factory):
    """(records, raw-multifasta-out.txt, processed-ests.txt) pintron_amd/bin/est-fact writes for the input, once per
    (input, setting) and process"""
    key = (source, retain)
    if key not in _product:
        gfa, efa = KL.real_inputs()[source]
        d = tmp_path_factory.mktemp("product_texts_%s_%d" % key)
        _product[key] = TL.program_texts(os.path.join(ROOT, "pintron_amd", "bin", "est-fact"), gfa, efa, retain, str(d))
    return _product[key]


@pytest.mark.parametrize("source,floor", [("c2", 151), ("issue13", 930)])
def test_the_products_records_to_its_two_files(gpu_ctx, tmp_path_factory, source, floor):
    gfa, efa = KL.real_inputs()[source]
    G = TL.original_genomic(gfa)
    for retain in (1, 0):
        rec, raw, pests = product_texts(source, retain, tmp_path_factory)
        units, _ = TL.units_of_blob(rec)
        headers, seqs = TL.entries(pests)
        assert len(units) == len(headers) >= floor
        for again in range(2):
            out, my_raw, my_pests = device(gpu_ctx, units, rec, headers, seqs, G)
            assert (out["verdict"] == TL.DONE).all()
            assert my_raw == raw and my_pests == pests, (retain, again)            # whole files


# ---- the plan form ----------------------------------------------------------------------------------------------------
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
    G = TL.original_genomic(gfa)
    idx = capi.Index(gpu_ctx, genomic)
    src = capi.TextSource(gpu_ctx, G)
    plan = capi.PairingPlan(gpu_ctx, idx, seqs, resident=resident, originals=originals)
    try:
        run_ladder(plan)
        finals = plan.fetch_final_factorizations()
        for retain in (1, 0):
            plan.run_units(q, U["pref_N"], retain)
            units, blob = plan.fetch_units()
            sizes = plan.run_texts(src, headers)
            got = plan.fetch_texts()
            assert sizes == (len(got[1]), len(got[2])) and plan.texts_ms() >= plan.texts_write_ms() > 0.0
            same(got, TL.texts(units, blob, headers, U["original"], G), "the restatement on the device's own units")
            same(got, device(gpu_ctx, units, blob, headers, U["original"], G), "the form without a plan")
            # each DONE unit against that EST's lines in the product's files
            theirs = TL.per_est(*product_texts(source, retain, tmp_path_factory))
            n_done = 0
            for i in np.nonzero(got[0]["verdict"] == TL.DONE)[0]:
                a, n, b, m = (int(got[0][f][i]) for f in ("raw_first", "raw_bytes", "pests_first", "pests_bytes"))
                assert theirs[int(q["est_index"][i])] == (got[1][a:a + n], got[2][b:b + m]), (i, U["units"][i])
                n_done += 1
            assert n_done == int((units["verdict"] == UL.U_ALIGNED).sum()) >= (140 if source == "c2" else 750)
            print("%s retain_externals %d: %d DONE units, raw %d bytes, pests %d bytes" % (source, retain, n_done, len(got[1]), len(got[2])))
            # units and finals are what they were behind the texts, and a rerun gives the same bytes
            again = plan.fetch_units()
            assert again[0].tobytes() == units.tobytes() and again[1] == blob
            assert all(a.tobytes() == b.tobytes() for a, b in zip(plan.fetch_final_factorizations(), finals))
            assert plan.run_texts(src, headers) == sizes
            same(plan.fetch_texts(), got, "a rerun")
        # units in reverse: the texts follow the units
        back, hback = q[::-1].copy(), headers[::-1]
        plan.run_units(back, U["pref_N"], 1)
        units, blob = plan.fetch_units()
        plan.run_texts(src, hback)
        want = plan.fetch_texts()
        same(want, TL.texts(units, blob, hback, U["original"], G), "in reverse")
        # a plan without originals prints the working sequences
        bare = capi.PairingPlan(gpu_ctx, idx, seqs, resident=resident)
        try:
            run_ladder(bare)
            bare.run_units(back, U["pref_N"], 1)
            u2, b2 = bare.fetch_units()
            bare.run_texts(src, hback)
            got2 = bare.fetch_texts()
            same(got2, TL.texts(u2, b2, hback, seqs, G), "without originals")
            assert got2[2] != want[2]
            if resident:                                    # `bare` ran in between: nothing of `plan` is left
                assert plan.fetch_texts_raw(len(q))[0] == capi.PGPU_EINVAL and "overwritten" in message(gpu_ctx)
                hb, hf = capi._offsets(hback)
                assert plan.run_texts_raw(src, hb, len(hb), hf) == capi.PGPU_EINVAL and "overwritten" in message(gpu_ctx)
                run_ladder(plan)
                plan.run_units(back, U["pref_N"], 1)
                plan.run_texts(src, hback)
            same(plan.fetch_texts(), want, "after another plan")
        finally:
            bare.close()
    finally:
        plan.close()
        src.close()
        idx.close()


def test_the_rules_of_the_seventh_rung(gpu_ctx):
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
    hb, hf = capi._offsets(headers)

    def fetch_refused():
        return plan.fetch_texts_raw(len(q), 1 << 20, 1 << 20)[0] == capi.PGPU_EINVAL and "run_texts first" in message(gpu_ctx)

    def run_refused(text, source=src, hb=hb, n=None, hf=hf):
        rc = plan.run_texts_raw(source, hb, len(hb) if n is None else n, hf)
        return (rc == capi.PGPU_EINVAL and text in message(gpu_ctx) and plan.text_bytes(0) == 0 and plan.text_bytes(1) == 0 and
                plan.texts_ms() == 0.0)
    try:
        assert fetch_refused() and run_refused("run_units")                                 # nothing ran yet
        run_ladder(plan)
        assert fetch_refused() and run_refused("run_units")
        plan.run_units(q, 11, 1)
        units = plan.fetch_units()
        finals = plan.fetch_final_factorizations()
        assert fetch_refused()
        # null pointers, bad offsets, a source of another context: refused, and the units stay
        assert plan.run_texts_raw(None, hb, len(hb), hf) == capi.PGPU_EINVAL and plan.run_texts_raw(src, hb, len(hb), None) == capi.PGPU_EINVAL
        assert plan.run_texts_raw(src, None, len(hb), hf) == capi.PGPU_EINVAL
        bad = hf.copy()
        bad[2] = bad[3] + 1
        assert run_refused("bad header offsets", hf=bad)
        assert run_refused("bad header offsets", n=len(hb) - 1)
        with capi.Context(0) as other_ctx:
            foreign = capi.TextSource(other_ctx, genomic)
            try:
                assert run_refused("another context", source=foreign)
                assert L_.pgpu_text_source_destroy(gpu_ctx.h, foreign.h) == capi.PGPU_EINVAL and "another context" in message(gpu_ctx)
            finally:
                foreign.close()
        assert fetch_refused()
        again = plan.fetch_units()
        assert again[0].tobytes() == units[0].tobytes() and again[1] == units[1]
        sizes = plan.run_texts(src, headers)
        want = plan.fetch_texts()
        same(want, TL.texts(units[0], units[1], headers, seqs, genomic))
        assert (want[0]["verdict"] == TL.DONE).any() or not (units[0]["verdict"] == UL.U_ALIGNED).any()
        assert plan.texts_ms() > 0.0 and L_.pgpu_pairing_plan_text_bytes(None, 0) == 0 and L_.pgpu_pairing_plan_texts_ms(None) == 0.0
        assert plan.text_bytes(2) == 0 and plan.text_bytes(-1) == 0
        if sizes[0]:
            assert plan.fetch_texts_raw(len(q), sizes[0] - 1, sizes[1])[0] == capi.PGPU_ENOSPC and message(gpu_ctx) == "text buffers too small"
        if sizes[1]:
            assert plan.fetch_texts_raw(len(q), sizes[0], sizes[1] - 1)[0] == capi.PGPU_ENOSPC
        # units and finals are unchanged behind the texts
        again = plan.fetch_units()
        assert again[0].tobytes() == units[0].tobytes() and again[1] == units[1]
        assert all(a.tobytes() == b.tobytes() for a, b in zip(plan.fetch_final_factorizations(), finals))
        # a refused run lowers the plan to the units, which stay
        assert run_refused("bad header offsets", hf=bad) and fetch_refused()
        assert plan.fetch_units()[1] == units[1]
        # a run of any earlier stage takes the texts with it
        for rerun in (lambda: plan.run_units(q, 11, 1), lambda: plan.run_final_factorizations(40),
                      lambda: plan.run_factorizations(*F.DEFAULTS), lambda: plan.run_candidates(15, 40),
                      lambda: plan.run_meg(**M.DEFAULTS), lambda: plan.run(15, 0.2)):
            plan.run_texts(src, headers)
            rerun()
            assert fetch_refused()
            run_ladder(plan)
            plan.run_units(q, 11, 1)
            assert plan.run_texts(src, headers) == sizes
            same(plan.fetch_texts(), want, "after a rerun of an earlier stage")
        # a run of zero units: the rung is reached, nothing to fetch
        assert plan.run_units_raw(None, 0, capi.unit_params(11, 1)) == capi.PGPU_OK
        assert plan.run_texts_raw(src, None, 0, None) == capi.PGPU_OK and plan.text_bytes(0) == 0 and plan.text_bytes(1) == 0
        assert L_.pgpu_pairing_plan_fetch_texts(gpu_ctx.h, plan.h, None, None, 0, None, 0) == capi.PGPU_OK
    finally:
        plan.close()
    # an empty plan
    for resident in (False, True):
        empty = capi.PairingPlan(gpu_ctx, idx, [], resident=resident)
        try:
            assert empty.run_texts_raw(src, None, 0, None) == capi.PGPU_EINVAL and "run_units" in message(gpu_ctx)
            assert empty.run_candidates(15, 40) == 0 and empty.run_factorizations(*F.DEFAULTS) == 0
            assert empty.run_final_factorizations(40) == 0
            assert empty.run_units_raw(None, 0, capi.unit_params(11, 1)) == capi.PGPU_OK
            assert empty.run_texts_raw(src, None, 0, None) == capi.PGPU_OK and empty.texts_ms() == 0.0
            assert L_.pgpu_pairing_plan_fetch_texts(gpu_ctx.h, empty.h, None, None, 0, None, 0) == capi.PGPU_OK
        finally:
            empty.close()
    src.close()
    idx.close()
