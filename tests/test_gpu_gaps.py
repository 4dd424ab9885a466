"""GPU: pgpu_index_gap_chains against the fixture whose border refinements are the reference's (the golden cases), against
today's route on the device (one plan of PGPU_DP_BORDERS jobs with the host logic of tests/gaps_lib.py around it), and
against the restatement (tests/gaps_lib.py) -- never against the library under test alone.  Every comparison is byte
equality."""
import ctypes as C

import numpy as np
import pytest

import gaps_lib as GL

pytestmark = pytest.mark.gpu

MESSAGE = ("bad gaps query (a range past its buffer, an empty EST, reserved != 0, no exon, an exon two queries share, a "
           "coordinate outside what it indexes, two adjacent exons out of order, or an EST gap longer than its genomic gap)")


@pytest.fixture(scope="module")
def golden(gpu_ctx):
    import pintron_amd.capi as capi
    gen, cases = GL.load_fixture()
    idx = capi.Index(gpu_ctx, gen)
    yield gen, cases, idx
    idx.close()


def pairs(cases):
    return [(c["est"], c["exons"]) for c in cases]


def golden_answers(cases):
    return [(GL.OK, c["verdict"], c["total"], c["n_kept"], c["exons_after"], c["steps"]) for c in cases]


def check(idx, ests, exons, q, want_arrays):
    out_exons, out_steps, res = idx.gap_chains(ests, exons, q)
    we, ws, wr = want_arrays
    for name, got, want in (("results", res, wr), ("steps", out_steps, ws), ("exons", out_exons, we)):
        if got.tobytes() != want.tobytes():
            bad = [i for i in range(len(got)) if got[i] != want[i]]
            raise AssertionError("%s differ at %d places, first %d: %r / %r" % (name, len(bad), bad[0], got[bad[0]], want[bad[0]]))
    return out_exons, out_steps, res


def test_every_golden_case_in_one_call_and_again(golden):
    gen, cases, idx = golden
    ests, exons, q = GL.batch_arrays(pairs(cases))
    first = check(idx, ests, exons, q, GL.expect_arrays(exons, golden_answers(cases)))
    assert idx.gap_chains_kernel_ms() > 0.0                    # the fixture's context has timing on
    again = idx.gap_chains(ests, exons, q)                     # the same call twice on one context gives the same bytes
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, again))


def test_golden_cases_on_a_loaded_index(golden, gpu_ctx, tmp_path):
    import pintron_amd.capi as capi
    gen, cases, idx = golden
    ests, exons, q = GL.batch_arrays(pairs(cases))
    path = str(tmp_path / "gaps.idx")
    idx.save(path)
    loaded = capi.Index(gpu_ctx, gen, load_from=path)
    try:
        check(loaded, ests, exons, q, GL.expect_arrays(exons, golden_answers(cases)))
    finally:
        loaded.close()


def test_two_thousand_fresh_queries_against_the_restatement_and_todays_route(golden, gpu_ctx):
    import pintron_amd.capi as capi
    gen, _, _ = golden
    g, batch = GL.make_world(2026, 2000, g=gen)                # its own ties planted over the fixture's
    want = [GL.gaps(est, g, ex) for est, ex in batch]
    assert {(w[0], w[1]) for w in want} == {(GL.OK, 0), (GL.OK, 1)}
    ests, exons, q = GL.batch_arrays(batch)
    idx = capi.Index(gpu_ctx, g)
    try:
        check(idx, ests, exons, q, GL.expect_arrays(exons, want))
        clock = {}
        assert GL.device_route(gpu_ctx, idx, g, batch, clock=clock) == want
        assert clock["jobs"] > 2000
    finally:
        idx.close()


# ---- hand-made edges ----------------------------------------------------------------------------------------------
def other_base(c):
    """a base that differs from c in either case"""
    u = bytes([c]).upper()
    return b"CGTA"[b"ACGT".index(u)] if u in b"ACGT" else 65


def substituted(s, places):
    s = bytearray(s)
    for p in places:
        s[p] = other_base(s[p])
    return bytes(s)


def hand_cases(gen):
    """named factorizations over the fixture's sequence, read only: (name, est, exons)"""
    glen = len(gen)
    cases = []

    def chain(name, at, parts):
        """exons and what lies between them, from `at` on: an int is an exon of that many bases, a tuple (EST gap, genomic
        gap) a junction"""
        est, exons = bytearray(), []
        for part in parts:
            if isinstance(part, int):
                exons.append((len(est), len(est) + part - 1, at, at + part - 1))
                est += gen[at:at + part]
                at += part
            else:
                gap, gap_t = part
                est += gap
                at += gap_t
        cases.append((name, bytes(est), exons))

    clean = 13_000                                                 # upper-case ACGT alone from here on, for the counted errors
    while any(c not in b"ACGT" for c in gen[clean:clean + 400]):
        clean += 50
    a = clean
    chain("p-equals-t", a, [20, (gen[a + 20:a + 30], 10), 20])                       # distance 0, the gap closes, merged
    chain("short-window", a, [20, (gen[a + 20:a + 25] + gen[a + 30:a + 35], 15), 20])      # gapT 15 < 2 gapP
    chain("short-window-errors", a, [20, (substituted(gen[a + 20:a + 25] + gen[a + 30:a + 35], [2, 7]), 15), 20])
    chain("run-of-three", a, [20, (b"", 0), 20, (b"", 3), 20])                      # three exons merged into one
    chain("run-then-far", a, [20, (b"", 2), 20, (b"", 3), 20, (b"", 4), 20])
    chain("gap3", a, [20, (b"", 3), 20])
    chain("gap4", a, [20, (b"", 4), 20])
    # totals of exactly 20 and 21: substitutions four apart in gaps that are their introns (10 + 10, 10 + 11)
    for name, k2 in (("total20", 10), ("total21", 11)):
        g1 = substituted(gen[a + 20:a + 62], range(1, 41, 4))
        g2 = substituted(gen[a + 82:a + 82 + 4 * k2 + 2], range(1, 4 * k2 + 1, 4))
        chain(name, a, [20, (g1, 42), 20, (g2, 4 * k2 + 2), 20])
    # an intron that begins at the first byte of the sequence: the donor lies in front of it (GEN_* = -1)
    first = bytes(gen[:6]) + bytes(gen[94:100])
    cases.append(("first-byte", b"AAAAA" + first + bytes(gen[100:120]), [(0, 4, -1, -1), (17, 36, 100, 119)]))
    cases.append(("first-byte-errors", b"AAAAA" + substituted(first, [3]) + bytes(gen[100:120]), [(0, 4, -1, -1), (17, 36, 100, 119)]))
    # ... and one that ends at the last: the acceptor lies behind it (GEN_* = the length), on the EST's last bytes
    last = bytes(gen[glen - 100:glen - 94]) + bytes(gen[glen - 6:])
    e = bytes(gen[glen - 120:glen - 100]) + last + b"CCCCC"
    cases.append(("last-byte", e, [(0, 19, glen - 120, glen - 101), (32, 36, glen, glen)]))
    e = bytes(gen[glen - 120:glen - 100]) + substituted(last, [8]) + b"CCCCC"
    cases.append(("last-byte-errors", e, [(0, 19, glen - 120, glen - 101), (32, 36, glen, glen)]))
    # the whole sequence as one intron of a gap of 64
    e = b"GG" + bytes(gen[:40]) + bytes(gen[glen - 24:]) + b"TT"
    cases.append(("whole-sequence", e, [(0, 1, -1, -1), (66, 67, glen, glen)]))
    # the caps: an EST gap of 64 / 65 bytes; 64 / 65 exons
    for n in (64, 65):
        chain("gap%d" % n, a, [20, (gen[a + 20:a + 20 + n], 300), 20])
        chain("exons%d" % n, a + 500, sum(([10, (gen[a:a + 1], 40)] for _ in range(n - 1)), []) + [10])
    chain("single", a, [50])
    return cases


def test_hand_made_edges_and_the_caps_in_one_batch(golden):
    gen, gold, idx = golden
    cases = hand_cases(gen)
    want = {name: GL.gaps(est, gen, exons) for name, est, exons in cases}
    for name, est, exons in cases:
        assert not GL.einval(len(est), len(gen), exons, [dict(est_off=0, est_len=len(est), first_exon=0, n_exons=len(exons), reserved=0)]), name
    m = GL.MERGED
    # the edges are the ones their names say
    assert want["p-equals-t"][1:4] == (0, 0, 1) and want["p-equals-t"][5] == [0, 1 | m]
    assert want["short-window"][1:3] == (0, 0) and want["short-window-errors"][1:3] == (0, 2)
    assert want["run-of-three"][3] == 1 and want["run-of-three"][5] == [0, m, m]
    assert want["run-of-three"][4][0][1::2] == (want["run-of-three"][4][2][1], want["run-of-three"][4][2][3])
    assert want["run-then-far"][3] == 2 and want["run-then-far"][5] == [0, m, m, 0]
    assert want["gap3"][5] == [0, m] and want["gap4"][5] == [0, 0]
    assert want["total20"][1:4] == (0, 20, 1) and want["total21"][1:4] == (1, 21, 0) and not any(s & m for s in want["total21"][5])
    assert want["first-byte"][1:3] == (0, 0) and want["first-byte-errors"][2] == 1
    assert want["last-byte"][1:3] == (0, 0) and want["last-byte-errors"][2] == 1
    assert want["whole-sequence"][1:3] == (0, 0) and want["whole-sequence"][5] == [0, 1]
    assert want["gap64"][0] == want["exons64"][0] == GL.OK and want["gap65"][0] == want["exons65"][0] == GL.ERANGE
    assert want["single"][:4] == (GL.OK, 0, 0, 1)
    # one call; every case between two ordinary ones, the refused ones unchanged, their neighbours exact
    ordinary = [c for c in gold if c["verdict"] == 0 and len(c["exons"]) >= 2][:3]
    batch, answers = [], []
    for k, (name, est, exons) in enumerate(cases):
        o = ordinary[k % 3]
        batch += [(o["est"], o["exons"]), (est, exons)]
        answers += [golden_answers([o])[0], want[name]]
    batch.append((ordinary[0]["est"], ordinary[0]["exons"]))
    answers.append(golden_answers(ordinary[:1])[0])
    ests, exons, q = GL.batch_arrays(batch)
    we, ws, wr = GL.expect_arrays(exons, answers)
    refused = wr["status"] == GL.ERANGE
    assert refused.sum() == 2 and not wr["verdict"][refused].any() and not wr["n_kept"][refused].any()
    check(idx, ests, exons, q, (we, ws, wr))
    # exons that no query names, in front and behind: copied, with step 0
    loose = np.array([(7, 9, 11, 13), (-1, -1, -1, -1)], dtype=exons.dtype)
    q_l = q.copy()
    q_l["first_exon"] += 1
    check(idx, ests, np.concatenate([loose[:1], exons, loose[1:]]), q_l,
          (np.concatenate([loose[:1], we, loose[1:]]), np.concatenate([[0], ws, [0]]).astype(np.uint8), wr))


def test_refusals_and_the_contract_of_the_entry(golden, gpu_ctx):
    import pintron_amd.capi as capi
    L = capi.lib()
    gen, cases, idx = golden
    glen = len(gen)
    some = [c for c in cases if c["verdict"] == 0 and len(c["exons"]) >= 3 and any(s & 0x7F for s in c["steps"])][:6]
    ests, exons, q = GL.batch_arrays(pairs(some))
    want = GL.expect_arrays(exons, golden_answers(some))
    n_ex = len(exons)
    f = L.pgpu_index_gap_chains

    def raw(ests_, e_, q_, n):
        """the call with its three outputs filled beforehand -> (rc, whether anything was written)"""
        oe = np.full(len(e_), 0x55, dtype=np.uint8).repeat(16).view(np.dtype(capi.FACTOR_DTYPE))
        ob = np.full(len(e_), 0x55, dtype=np.uint8)
        orr = np.full(16 * max(n, 1), 0x55, dtype=np.uint8).view(np.dtype(capi.GAPS_RESULT_DTYPE))
        rc = f(gpu_ctx.h, idx.h, ests_, len(ests_), e_.ctypes.data_as(C.POINTER(capi.Factor)), len(e_),
               q_.ctypes.data_as(C.POINTER(capi.GapsQuery)), n, oe.ctypes.data_as(C.POINTER(capi.Factor)),
               ob.ctypes.data_as(C.POINTER(C.c_uint8)), orr.ctypes.data_as(C.POINTER(capi.GapsResult)))
        untouched = all((x.view(np.uint8) == 0x55).all() for x in (oe, ob, orr))
        return rc, untouched, (oe, ob, orr)

    def rc_of(mod_q=None, mod_e=None, ests_=None):
        q2, e2 = q.copy(), exons.copy()
        if mod_q:
            mod_q(q2)
        if mod_e:
            mod_e(e2)
        b = ests if ests_ is None else ests_
        rc, untouched, _ = raw(b, e2, q2, len(q2))
        assert (rc == capi.PGPU_EINVAL) == GL.einval(len(b), glen, e2, q2) and rc in (capi.PGPU_OK, capi.PGPU_EINVAL)
        if rc == capi.PGPU_EINVAL:
            assert L.pgpu_last_error(gpu_ctx.h).decode() == MESSAGE and idx.gap_chains_kernel_ms() == 0.0 and untouched
        return rc

    def put(field, i, value):
        def mod(x):
            x[field][i] = value
        return mod
    f1, n1 = int(q[1]["first_exon"]), int(q[1]["n_exons"])
    bad_q = [put("n_exons", 2, 0), put("n_exons", len(q) - 1, int(q[-1]["n_exons"]) + 1), put("first_exon", 3, len(exons)),
             put("first_exon", 3, 0xFFFFFFFF), put("est_off", 1, len(ests)), put("est_off", 1, 1 << 40), put("est_len", 1, 0xFFFFFFFF),
             put("est_len", 1, 0x80000000), put("est_len", 1, 0), put("reserved", 4, 1), put("first_exon", 1, f1 - 1),
             put("n_exons", 0, int(q[0]["n_exons"]) + 1)]
    for k, mod in enumerate(bad_q):
        check(idx, ests, exons, q, want)                                          # a slot for the refusal to reset
        assert idx.gap_chains_kernel_ms() > 0.0
        assert rc_of(mod_q=mod) == capi.PGPU_EINVAL, k
    nxt = exons[f1 + 1]
    gap_p = int(nxt["EST_start"]) - int(exons[f1]["EST_end"]) - 1
    bad_e = [put("EST_start", f1 + 1, -2), put("EST_end", f1 + 1, int(q[1]["est_len"]) + 1), put("GEN_start", f1 + 1, -2),
             put("GEN_end", f1 + 1, glen + 1),
             put("EST_end", f1, int(nxt["EST_start"])), put("GEN_end", f1, int(nxt["GEN_start"])),             # out of order
             put("GEN_end", f1, int(nxt["GEN_start"]) - gap_p)]                                                 # gapP == gapT + 1
    for k, mod in enumerate(bad_e):
        assert rc_of(mod_e=mod) == capi.PGPU_EINVAL, k
    assert rc_of(mod_e=put("GEN_end", f1, int(nxt["GEN_start"]) - gap_p - 1)) == capi.PGPU_OK                  # gapP == gapT
    assert rc_of(ests_=ests[:-1]) == capi.PGPU_EINVAL                             # the last EST runs past the buffer
    # the refusal is repeated after a good call
    for _ in range(2):
        check(idx, ests, exons, q, want)
        assert idx.gap_chains_kernel_ms() > 0.0
        assert rc_of(mod_q=put("reserved", 0, 1)) == capi.PGPU_EINVAL
    # null pointers: a bare refusal, the message stays; n == 0
    oe, ob = np.zeros_like(exons), np.full(n_ex, 9, dtype=np.uint8)
    orr = np.zeros(len(q), dtype=np.dtype(capi.GAPS_RESULT_DTYPE))
    ep, qp = exons.ctypes.data_as(C.POINTER(capi.Factor)), q.ctypes.data_as(C.POINTER(capi.GapsQuery))
    oep, obp, orp = oe.ctypes.data_as(C.POINTER(capi.Factor)), ob.ctypes.data_as(C.POINTER(C.c_uint8)), orr.ctypes.data_as(C.POINTER(capi.GapsResult))
    check(idx, ests, exons, q, want)
    for args in ((None, ests, ep, qp, oep, obp, orp), (idx.h, None, ep, qp, oep, obp, orp), (idx.h, ests, None, qp, oep, obp, orp),
                 (idx.h, ests, ep, None, oep, obp, orp), (idx.h, ests, ep, qp, None, obp, orp), (idx.h, ests, ep, qp, oep, None, orp),
                 (idx.h, ests, ep, qp, oep, obp, None)):
        ih, es, e_, q_, oe_, ob_, or_ = args
        assert f(gpu_ctx.h, ih, es, len(ests), e_, n_ex, q_, len(q), oe_, ob_, or_) == capi.PGPU_EINVAL
        assert L.pgpu_last_error(gpu_ctx.h).decode() == MESSAGE                   # of the refusal before: untouched
        assert idx.gap_chains_kernel_ms() == 0.0
    assert f(None, idx.h, ests, len(ests), ep, n_ex, qp, len(q), oep, obp, orp) == capi.PGPU_EINVAL
    check(idx, ests, exons, q, want)
    assert idx.gap_chains_kernel_ms() > 0.0
    assert f(gpu_ctx.h, idx.h, ests, len(ests), ep, n_ex, None, 0, oep, obp, None) == capi.PGPU_OK       # n == 0: a copy
    assert oe.tobytes() == exons.tobytes() and not ob.any() and idx.gap_chains_kernel_ms() == 0.0
    assert f(gpu_ctx.h, idx.h, None, 0, None, 0, None, 0, None, None, None) == capi.PGPU_OK
    check(idx, ests, exons, q, want)                                              # the context still answers


def test_without_timing_the_answers_are_the_same(golden):
    import pintron_amd.capi as capi
    gen, cases, _ = golden
    ests, exons, q = GL.batch_arrays(pairs(cases[:80]))
    want = GL.expect_arrays(exons, golden_answers(cases[:80]))
    with capi.Context(0) as ctx:
        idx = capi.Index(ctx, gen)
        check(idx, ests, exons, q, want)
        assert idx.gap_chains_kernel_ms() > 0.0
        ctx.L.pgpu_set_timing(ctx.h, 0)
        check(idx, ests, exons, q, want)
        assert idx.gap_chains_kernel_ms() == 0.0
        idx.close()
