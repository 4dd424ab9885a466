"""GPU: pgpu_index_clean_chains against what the reference's six cleaning routines left (the golden cases), against today's
route on the device (PGPU_DP_ALIGN and PGPU_DP_KBAND plans with the host logic of tests/clean_lib.py in between), and
against the restatement (tests/clean_lib.py) -- never against the library under test alone.  Every comparison is byte
equality."""
import ctypes as C
import math

import numpy as np
import pytest

import clean_lib as CL
import oracle_lib as O
import refine_lib as RL

pytestmark = pytest.mark.gpu

MESSAGE = ("bad clean query (a range past its buffer, an empty EST, reserved != 0, no exon, an exon two queries share, a "
           "coordinate outside what it indexes, or an end exon that begins in front of or ends behind its sequence)")


@pytest.fixture(scope="module")
def golden(gpu_ctx):
    import pintron_amd.capi as capi
    gen, cases = CL.load_fixture()
    idx = capi.Index(gpu_ctx, gen)
    yield gen, cases, idx
    idx.close()


def triples(cases):
    return [(c["est"], c["exons"], c["thr"]) for c in cases]


def golden_answers(cases):
    return [(CL.OK, c["verdict"], c["first"], c["n"], c["exons_after"], c["marks"]) for c in cases]


def check(idx, ests, exons, q, want_arrays):
    out_exons, out_marks, res = idx.clean_chains(ests, exons, q)
    we, wm, wr = want_arrays
    for name, got, want in (("results", res, wr), ("marks", out_marks, wm), ("exons", out_exons, we)):
        if got.tobytes() != want.tobytes():
            bad = [i for i in range(len(got)) if got[i] != want[i]]
            raise AssertionError("%s differ at %d places, first %d: %r / %r" % (name, len(bad), bad[0], got[bad[0]], want[bad[0]]))
    return out_exons, out_marks, res


def test_every_golden_case_in_one_call_and_again(golden):
    gen, cases, idx = golden
    ests, exons, q = CL.batch_arrays(triples(cases))
    first = check(idx, ests, exons, q, CL.expect_arrays(exons, golden_answers(cases)))
    assert idx.clean_chains_kernel_ms() > 0.0                  # the fixture's context has timing on
    again = idx.clean_chains(ests, exons, q)                   # the same call twice gives the same bytes
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, again))


def test_golden_cases_by_todays_route(golden, gpu_ctx):
    """an ALIGN plan with p0 for the heads, one for the tails, then a KBAND `tail = 1` plan, with the host logic of clean_lib"""
    gen, cases, idx = golden
    assert CL.device_route(gpu_ctx, gen, triples(cases)) == golden_answers(cases)


# ---- hand-made edges ----------------------------------------------------------------------------------------------
def other_base(c):
    return b"CGTA"[b"ACGT".index(c)]


def substituted(s, places):
    s = bytearray(s)
    for p in places:
        s[p] = other_base(s[p])
    return bytes(s)


def hand_world():
    """a sequence of 60 000 seeded random bases with what the edges need written into it, one region after the other:
    (sequence, the named candidates (name, est, exons, threshold), three ordinary candidates)"""
    rng = np.random.default_rng(77)
    g = bytearray(RL.rnd(rng, 60_000))
    glen = len(g)
    cases = []
    free = [100]

    def take(n):
        """the start of the next n untouched bases (with room for a site on either side)"""
        base = free[0] + 10
        free[0] = base + n + 10
        assert free[0] < glen - 100
        return base

    def add(name, est, exons, thr=20.0):
        cases.append((name, bytes(est), [tuple(e) for e in exons], thr))

    def two(name, head, tail, thr=20.0, est_head=None, est_tail=None):
        """two exons given by their extents on the sequence, the EST their bytes (or what is given instead)"""
        eh = bytes(g[head[0]:head[1] + 1]) if est_head is None else est_head
        et = bytes(g[tail[0]:tail[1] + 1]) if est_tail is None else est_tail
        add(name, eh + et, [(0, len(eh) - 1, head[0], head[1]), (len(eh), len(eh) + len(et) - 1, tail[0], tail[1])], thr)

    p = take(100)
    front = (p, p + 99)                                          # an ordinary exon in front of the one under test ...
    p = take(40)
    p = take(100)
    back = (p, p + 99)                                           # ... and one behind it
    h = front[0] + 110                                           # between the two
    # six / seven matching columns at the head, eleven / twelve at the tail
    two("head6", (h, h + 5), back)
    two("head7", (h, h + 6), back)
    t = take(20)
    two("tail11", front, (t, t + 10))
    two("tail12", front, (t, t + 11))
    # (a tail that matches throughout is never dropped, for its new end is its old one: the test that comes one column late
    # shows where a column that does not match stands in front of the run -- behind ten matches it is walked over and the
    # exon ends in front of its start, behind eleven the walk has stopped)
    for n in (10, 11):
        piece = bytes(g[t:t + n + 1])
        two("tail-x%d" % n, front, (t, t + n), est_tail=bytes([other_base(piece[0])]) + piece[1:])
    # single exon; head dropped from two exons
    p = take(100)
    add("single", g[p:p + 100], [(0, 99, p, p + 99)])
    two("drop-head", (h, h + 39), back, est_head=RL.rnd(rng, 40))
    # end exon of 64 / 65 EST bytes (one substitution: no identity shortcut)
    p = take(65)
    for n in (64, 65):
        add("est%d" % n, substituted(g[p:p + n], [n // 2]), [(0, n - 1, p, p + n - 1)])
    # length difference 31 / 32 above 64 EST bytes, either way
    p = take(140)
    for d in (31, 32):
        add("longer-gen%d" % d, g[p:p + 100], [(0, 99, p, p + 99 + d)])
        add("longer-est%d" % d, g[p:p + 100 + d], [(0, 99 + d, p, p + 99)])
    # 31 / 32 spaced substitutions in 400 bases
    p = take(400)
    for k in (31, 32):
        add("subst%d" % k, substituted(g[p:p + 400], range(5, 5 + 12 * k, 12)), [(0, 399, p, p + 399)])
    # 4096 / 4097 bytes (the threshold lets step 4 reject what step 5 would refuse), with and without the identity shortcut
    low = 1e-9
    p = take(4097)
    for n in (4096, 4097):
        add("id%d" % n, g[p:p + n], [(0, n - 1, p, p + n - 1)], low)
        add("band%d" % n, substituted(g[p:p + n], [2000]), [(0, n - 1, p, p + n - 1)], low)
        add("gen%d" % n, g[p:p + 64], [(0, 63, p, p + n - 1)], low)               # 64 EST bytes over n genomic ones
    # gap closing on either row: bases missing from / added to the tail a few columns from its end, inside a run of one base
    # (the pull succeeds), in front of another base (a mismatch stops it), one or two of them (a run of gaps)
    t0 = take(60)
    g[t0 + 49:t0 + 56] = b"AAAAAAA"
    tail = bytes(g[t0:t0 + 60])
    for cut in (50, 52, 54, 57):
        for k in (1, 2):
            two("tail-del%d-%d" % (cut, k), front, (t0, t0 + 59), est_tail=tail[:cut] + tail[cut + k:])
            two("tail-ins%d-%d" % (cut, k), front, (t0, t0 + 59), est_tail=tail[:cut] + tail[cut - 1:cut] * k + tail[cut:])
            two("tail-insx%d-%d" % (cut, k), front, (t0, t0 + 59), est_tail=tail[:cut] + bytes([other_base(tail[cut])]) * k + tail[cut:])
    # external exons of 9 / 10 / 19 / 20 bytes between sites of either case, a C at +2, no site; equal but for case or an N
    for i, (don, acc) in enumerate(((b"GT", b"AG"), (b"gt", b"ag"), (b"GC", b"AG"), (b"gC", b"aG"), (b"GA", b"AG"), (b"GT", b"AC"))):
        for n in (9, 10, 19, 20):
            h0 = take(n + 300 + n)
            b0 = h0 + n + 100
            tl = b0 + 200
            g[h0 + n:h0 + n + 2], g[b0 - 2:b0] = don, acc                         # the intron behind the short head
            g[b0 + 100:b0 + 102], g[tl - 2:tl] = don, acc                         # the intron in front of the short tail
            two("ext-head%d-%d" % (n, i), (h0, h0 + n - 1), (b0, b0 + 99))
            two("ext-tail%d-%d" % (n, i), (b0, b0 + 99), (tl, tl + n - 1))
            if i == 0:
                piece = bytes(g[h0:h0 + n])
                # (in the exon's last byte: the head's walk stops at its first six bytes and trims nothing)
                two("ext-case%d" % n, (h0, h0 + n - 1), (b0, b0 + 99), est_head=piece[:-1] + piece[-1:].lower())
                two("ext-n%d" % n, (h0, h0 + n - 1), (b0, b0 + 99), est_head=piece[:-1] + b"N")
    # an exon that ends on the sequence's last byte, and one byte in front of it: the site behind it lies outside
    add("last-byte", g[glen - 15:], [(0, 14, glen - 15, glen - 1)])
    add("last-but-one", g[glen - 16:glen - 1], [(0, 14, glen - 16, glen - 2)])
    two("tail-at-the-end", front, (glen - 15, glen - 1))
    # dust: the threshold on an exon's score and one ulp below it
    p = take(100)
    score = O.dust_score(bytes(g[p:p + 100]))
    add("dust-on", g[p:p + 100], [(0, 99, p, p + 99)], score)
    add("dust-below", g[p:p + 100], [(0, 99, p, p + 99)], math.nextafter(score, 0.0))

    # five exons of 60 bases between canonical sites, some of them a (CA)n repeat (dust 2.4) or with every third base of
    # their middle changed (twelve errors against a bound of three; the outer 12 and 14 bases stay, for the end exons):
    # every exon flagged, the first / middle / last one, two that leave three equal runs
    def five(name, repeats=(), noisy=(), thr=2.0):
        base = take(5 * 160)
        est, exons = b"", []
        for k in range(5):
            a = base + 160 * k
            if k in repeats:
                g[a:a + 60] = b"CA" * 30
            g[a - 2:a], g[a + 60:a + 62] = b"AG", b"GT"
            piece = bytes(g[a:a + 60])
            exons.append((len(est), len(est) + 59, a, a + 59))
            est += substituted(piece, range(12, 46, 3)) if k in noisy else piece
        add(name, est, exons, thr)
    for nm, flagged in (("all", (0, 1, 2, 3, 4)), ("first", (0,)), ("middle", (2,)), ("last", (4,)), ("tie", (1, 3))):
        five("dust-" + nm, repeats=flagged)
        five("noisy-" + nm, noisy=flagged)
    # the K-band cap: a genomic length of 1 033 / 1 034 in the middle
    a, m, b = take(100), take(1034), take(100)
    for n in (1033, 1034):
        e = bytes(g[a:a + 100]) + bytes(g[m:m + n]) + bytes(g[b:b + 100])
        add("kband%d" % n, e, [(0, 99, a, a + 99), (100, 99 + n, m, m + n - 1), (100 + n, 199 + n, b, b + 99)])
    # 64 / 65 exons of 30 bases
    p = take(65 * 50)
    for n in (64, 65):
        est, exons = b"", []
        for i in range(n):
            a = p + 50 * i
            exons.append((len(est), len(est) + 29, a, a + 29))
            est += bytes(g[a:a + 30])
        add("exons%d" % n, est, exons)
    # cover 7/20 and 6/20 of the EST
    p = take(35)
    for n in (35, 30):
        add("cover%d" % n, bytes(g[p:p + n]) + RL.rnd(rng, 100 - n), [(0, n - 1, p, p + n - 1)])
    # verdicts 1 and 2
    a, b = take(50), take(50)
    add("v1-before", g[a:a + 50], [(-1, 49, a, a + 49)])
    add("v1-behind", g[a:a + 50], [(50, 50, a, a + 49)])
    add("v2-reversed", g[a:a + 50] + g[b:b + 50], [(0, 49, a, a + 49), (99, 50, b, b + 49)])
    add("v2-order", g[a:a + 50] + g[b:b + 50], [(50, 99, b, b + 49), (0, 49, a, a + 49)])
    # three ordinary candidates, kept whole or trimmed
    ordinary = []
    while len(ordinary) < 3:
        est, exons, thr, end = CL.make_case(rng, g, free[0])
        free[0] = end + 20
        assert free[0] < glen - 100
        if CL.clean(est, bytes(g), exons, 20.0)[:2] == (CL.OK, 0):
            ordinary.append((est, exons, 20.0))
    return bytes(g), cases, ordinary


@pytest.fixture(scope="module")
def hand(gpu_ctx):
    import pintron_amd.capi as capi
    gen, cases, ordinary = hand_world()
    idx = capi.Index(gpu_ctx, gen)
    yield gen, cases, ordinary, idx
    idx.close()


def test_hand_made_edges(hand):
    gen, cases, ordinary, idx = hand
    want = {}
    infos = {}
    for name, est, exons, thr in cases:
        infos[name] = {}
        want[name] = CL.clean(est, gen, exons, thr, info=infos[name])
    st = {n: w[:2] for n, w in want.items()}
    mk = {n: w[5] for n, w in want.items()}
    # the edges are the ones their names say
    assert mk["head6"][0] == CL.M_ENDPOINTS and mk["head7"][0] == CL.M_EXTERNAL
    assert mk["tail11"][1] == mk["tail12"][1] == CL.M_EXTERNAL
    assert mk["tail-x10"][1] == CL.M_ENDPOINTS and mk["tail-x11"][1] == CL.M_EXTERNAL
    assert st["single"] == (CL.OK, 0) and mk["drop-head"][0] == CL.M_ENDPOINTS and st["drop-head"] == (CL.OK, 0)
    assert st["est64"] == st["est65"] == (CL.OK, 0) and infos["est65"]["band"] and not infos["est64"]["band"]
    assert st["longer-gen31"][0] == st["longer-est31"][0] == CL.OK and st["longer-gen32"][0] == st["longer-est32"][0] == CL.ERANGE
    assert st["subst31"][0] == CL.OK and st["subst32"][0] == CL.ERANGE
    assert st["id4096"] == st["band4096"] == (CL.OK, 5) and st["gen4096"][0] == CL.OK
    assert st["id4097"][0] == st["band4097"][0] == st["gen4097"][0] == CL.ERANGE
    closing = [n for n in want if n.startswith("tail-") and infos[n].get("gap_closing")]
    assert len(closing) >= 8 and len({want[n][4][1] for n in closing}) >= 4, closing
    assert {n[:8] for n in closing} >= {"tail-del", "tail-ins"}
    for n in (9, 10, 19, 20):
        kept = {i for i in range(6) if not mk["ext-head%d-%d" % (n, i)][0] & CL.M_EXTERNAL}
        assert kept == {9: set(), 10: {0, 1, 2, 3}, 19: {0, 1, 2, 3}, 20: set(range(6))}[n], (n, kept)
        kept = {i for i in range(6) if not mk["ext-tail%d-%d" % (n, i)][1] & CL.M_EXTERNAL}
        assert kept == {9: set(), 10: {0, 1, 2, 3}, 19: {0, 1, 2, 3}, 20: set(range(6))}[n], (n, kept)
    assert mk["ext-head10-0"][0] == mk["ext-head19-0"][0] == 0                  # kept, and with one byte that differs dropped
    assert mk["ext-case10"][0] == mk["ext-case19"][0] == mk["ext-n10"][0] == mk["ext-n19"][0] == CL.M_EXTERNAL
    assert mk["ext-case20"][0] == mk["ext-n20"][0] == 0
    assert st["last-byte"] == st["last-but-one"] == (CL.OK, 4) and st["tail-at-the-end"] == (CL.OK, 0)
    assert st["dust-on"] == (CL.OK, 0) and st["dust-below"] == (CL.OK, 5)
    assert st["dust-all"] == (CL.OK, 5) and want["dust-first"][2:4] == (1, 4) and want["dust-middle"][2:4] == (0, 2)
    assert want["dust-last"][2:4] == (0, 4) and want["dust-tie"][2:4] == (0, 1) and infos["dust-tie"]["tie"]
    assert st["noisy-all"] == (CL.OK, 6) and want["noisy-first"][2:4] == (1, 4) and want["noisy-middle"][2:4] == (0, 2)
    assert want["noisy-last"][2:4] == (0, 4) and want["noisy-tie"][2:4] == (0, 1) and infos["noisy-tie"]["tie"]
    assert all(m in (0, CL.M_NOISY) for n in want if n.startswith("noisy-") for m in mk[n])
    assert st["kband1033"] == (CL.OK, 0) and st["kband1034"][0] == CL.ERANGE
    assert st["exons64"] == (CL.OK, 0) and st["exons65"][0] == CL.ERANGE
    assert st["cover35"] == (CL.OK, 0) and st["cover30"] == (CL.OK, 7)
    assert st["v1-before"] == st["v1-behind"] == (CL.OK, 1) and st["v2-reversed"] == st["v2-order"] == (CL.OK, 2)
    refused = [n for n, w in want.items() if w[0] == CL.ERANGE]
    assert len(refused) == 8, refused
    # one call; every candidate between two ordinary ones, and an exon nobody names in front and behind
    batch = []
    for k, (name, est, exons, thr) in enumerate(cases):
        batch += [ordinary[k % 3], (est, exons, thr)]
    batch.append(ordinary[0])
    answers = [CL.clean(est, gen, exons, thr) for est, exons, thr in batch]
    assert all(a[:2] == (CL.OK, 0) for a in answers[::2])
    ests, exons, q = CL.batch_arrays(batch)
    we, wm, wr = CL.expect_arrays(exons, answers)
    check(idx, ests, exons, q, (we, wm, wr))
    loose = np.array([(7, 9, 11, 13), (-1, -1, -1, -1)], dtype=exons.dtype)
    q_l = q.copy()
    q_l["first_exon"] += 1
    check(idx, ests, np.concatenate([loose[:1], exons, loose[1:]]), q_l,
          (np.concatenate([loose[:1], we, loose[1:]]), np.concatenate([[0], wm, [0]]).astype(np.uint8), wr))


def test_one_long_end_exon_in_a_large_batch(hand):
    """4096 genomic bytes under lev_wave<ALIGN> make the workspace of a wave 266 KB: with 3 000 queries beside it the grid
    is cut to what 256 MB of workspace allow, and the answers are what they are in a small batch"""
    gen, cases, ordinary, idx = hand
    named = {name: (est, exons, thr) for name, est, exons, thr in cases}
    batch = [ordinary[k % 3] for k in range(1500)] + [named["gen4096"], named["id4096"], named["band4096"]] + \
            [ordinary[k % 3] for k in range(1500)]
    one = {id(c): CL.clean(c[0], gen, c[1], c[2]) for c in ordinary + [named["gen4096"], named["id4096"], named["band4096"]]}
    ests, exons, q = CL.batch_arrays(batch)
    check(idx, ests, exons, q, CL.expect_arrays(exons, [one[id(c)] for c in batch]))


def test_refusals_and_the_contract_of_the_entry(golden, gpu_ctx, tmp_path):
    import pintron_amd.capi as capi
    L = capi.lib()
    gen, cases, idx = golden
    glen = len(gen)
    some = [c for c in cases if c["verdict"] == 0 and len(c["exons"]) >= 3 and c["exons"][0][0] > 0][:6]
    ests, exons, q = CL.batch_arrays(triples(some))
    want = CL.expect_arrays(exons, golden_answers(some))

    def rc_of(mod_q=None, mod_e=None, ests_=None):
        q2, e2 = q.copy(), exons.copy()
        if mod_q:
            mod_q(q2)
        if mod_e:
            mod_e(e2)
        b = ests if ests_ is None else ests_
        rc = idx.clean_chains_raw(b, e2, q2, len(q2))[0]
        assert (rc == capi.PGPU_EINVAL) == CL.einval(len(b), glen, e2, q2) and rc in (capi.PGPU_OK, capi.PGPU_EINVAL)
        if rc == capi.PGPU_EINVAL:
            assert L.pgpu_last_error(gpu_ctx.h).decode() == MESSAGE and idx.clean_chains_kernel_ms() == 0.0
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
        assert rc_of(mod_q=mod) == capi.PGPU_EINVAL, k
    last = f1 + n1 - 1
    bad_e = [put("EST_start", f1 + 1, -2), put("EST_end", f1 + 1, int(q[1]["est_len"]) + 1), put("GEN_start", f1 + 1, -2),
             put("GEN_end", f1 + 1, glen + 1),
             # the my_asserts of handle_endpoints
             put("EST_start", f1, -1), put("GEN_start", f1, -1), put("EST_end", last, int(q[1]["est_len"])), put("GEN_end", last, glen)]
    for k, mod in enumerate(bad_e):
        assert rc_of(mod_e=mod) == capi.PGPU_EINVAL, k
    assert rc_of(ests_=ests[:-1]) == capi.PGPU_EINVAL                             # the last EST runs past the buffer
    assert rc_of(mod_q=put("complexity_threshold", 2, -5.0)) == capi.PGPU_OK      # compared, never validated
    assert rc_of(mod_e=put("EST_end", f1, int(exons[f1 + 1]["EST_start"]) + 3)) == capi.PGPU_OK      # out of order: verdict 2
    # null pointers: a bare refusal, the message stays; n == 0
    n_ex = len(exons)
    assert rc_of(mod_q=put("reserved", 0, 1)) == capi.PGPU_EINVAL
    oe, om = np.zeros_like(exons), np.full(n_ex, 9, dtype=np.uint8)
    orr = np.zeros(len(q), dtype=np.dtype(capi.CLEAN_RESULT_DTYPE))
    ep, qp = exons.ctypes.data_as(C.POINTER(capi.Factor)), q.ctypes.data_as(C.POINTER(capi.CleanQuery))
    oep, omp, orp = oe.ctypes.data_as(C.POINTER(capi.Factor)), om.ctypes.data_as(C.POINTER(C.c_uint8)), orr.ctypes.data_as(C.POINTER(capi.CleanResult))
    f = L.pgpu_index_clean_chains
    check(idx, ests, exons, q, want)
    assert idx.clean_chains_kernel_ms() > 0.0
    for args in ((None, ests, ep, qp, oep, omp, orp), (idx.h, None, ep, qp, oep, omp, orp), (idx.h, ests, None, qp, oep, omp, orp),
                 (idx.h, ests, ep, None, oep, omp, orp), (idx.h, ests, ep, qp, None, omp, orp), (idx.h, ests, ep, qp, oep, None, orp),
                 (idx.h, ests, ep, qp, oep, omp, None)):
        ih, es, e_, q_, oe_, om_, or_ = args
        assert f(gpu_ctx.h, ih, es, len(ests), e_, n_ex, q_, len(q), oe_, om_, or_) == capi.PGPU_EINVAL
        assert L.pgpu_last_error(gpu_ctx.h).decode() == MESSAGE                   # of the refusal before: untouched
        assert idx.clean_chains_kernel_ms() == 0.0
    assert f(None, idx.h, ests, len(ests), ep, n_ex, qp, len(q), oep, omp, orp) == capi.PGPU_EINVAL
    check(idx, ests, exons, q, want)
    assert idx.clean_chains_kernel_ms() > 0.0
    assert f(gpu_ctx.h, idx.h, ests, len(ests), ep, n_ex, None, 0, oep, omp, None) == capi.PGPU_OK       # n == 0: a copy
    assert oe.tobytes() == exons.tobytes() and not om.any() and idx.clean_chains_kernel_ms() == 0.0
    assert f(gpu_ctx.h, idx.h, None, 0, None, 0, None, 0, None, None, None) == capi.PGPU_OK
    check(idx, ests, exons, q, want)                                              # the context still answers
    # a loaded index
    path = str(tmp_path / "clean.idx")
    idx.save(path)
    loaded = capi.Index(gpu_ctx, gen, load_from=path)
    check(loaded, ests, exons, q, want)
    loaded.close()


def test_without_timing_the_answers_are_the_same(golden):
    import pintron_amd.capi as capi
    gen, cases, _ = golden
    ests, exons, q = CL.batch_arrays(triples(cases[:60]))
    want = CL.expect_arrays(exons, golden_answers(cases[:60]))
    with capi.Context(0) as ctx:
        idx = capi.Index(ctx, gen)
        check(idx, ests, exons, q, want)
        assert idx.clean_chains_kernel_ms() > 0.0
        ctx.L.pgpu_set_timing(ctx.h, 0)
        check(idx, ests, exons, q, want)
        assert idx.clean_chains_kernel_ms() == 0.0
        idx.close()


BATCH, DISTINCT, SAMPLE = 20_000, 2_500, 2_000
SWEEP = (20.0, 4.0, 2.0, 1.0, 0.5, 0.32, 0.3, 0.25)


def test_twenty_thousand_generated_queries_in_one_call(golden):
    """one batch of 20 000 queries: 2 500 generated candidates planted at random places of a copy of the sequence (later
    ones over earlier ones), each under eight complexity thresholds.  The restatement is a Python loop: a seeded sample of
    2 000 queries is compared, and every result must be a well-formed one."""
    import pintron_amd.capi as capi
    gen, _, _ = golden
    rng = np.random.default_rng(2025)
    g = bytearray(gen[:600_000])
    bases = []
    pos = 300
    for k in range(DISTINCT):
        est, exons, thr, end = CL.make_case(rng, g, pos, aim=CL.AIMS[k % len(CL.AIMS)], k=k)
        bases.append((est, exons))
        pos = end + 20 if end + 6000 < len(g) else 300 + int(rng.integers(0, 3000))
    g = bytes(g)
    batch = [(est, exons, thr) for est, exons in bases for thr in SWEEP]
    assert len(batch) == BATCH
    ests, exons, q = CL.batch_arrays(batch)
    with capi.Context(0) as ctx:
        idx = capi.Index(ctx, g)
        out_exons, out_marks, res = idx.clean_chains(ests, exons, q)
        idx.close()
    ok = res["status"] == CL.OK
    assert np.all(ok | (res["status"] == CL.ERANGE)) and np.all(res["verdict"] <= 7) and np.all((out_marks & 0xE0) == 0)
    kept = ok & ((res["verdict"] == 0) | (res["verdict"] == 7))
    assert np.all(res["n_kept"][~kept] == 0) and np.all(res["first_kept"][~kept] == 0)
    assert np.all(res["n_kept"][kept] >= 1) and np.all(res["first_kept"][kept] + res["n_kept"][kept] <= q["n_exons"][kept])
    sample = np.sort(rng.permutation(BATCH)[:SAMPLE])
    verdicts = set()
    for i in sample:
        est, ex, thr = batch[int(i)]
        want = CL.clean(est, g, ex, thr)
        k, n = int(q[i]["first_exon"]), len(ex)
        got = (int(res[i]["status"]), int(res[i]["verdict"]), int(res[i]["first_kept"]), int(res[i]["n_kept"]),
               [tuple(int(v) for v in e) for e in out_exons[k:k + n]], out_marks[k:k + n].tolist())
        assert got == want, (int(i), got, want)
        verdicts.add((want[0], want[1]))
    assert {(CL.OK, v) for v in range(8)} <= verdicts, verdicts
