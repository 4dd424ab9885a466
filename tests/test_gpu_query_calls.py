"""GPU: what the host side of every query on the resident index promises around its kernels
(pintron_amd/csrc/pgpu_query_call.h), entry by entry on one sequence of 700 bases with two or three queries each:
the millisecond slot is set with timing on and 0.0 without it, with the same answers; a call refused with PGPU_EINVAL
resets the slot and leaves its message; the context answers the same afterwards; an empty call is PGPU_OK with the slot
at 0.  The same for the index forms of the four device stages (pgpu_index_candidates, pgpu_index_factorizations,
pgpu_index_final_factorizations, pgpu_unit_records).  For pgpu_index_find also the PGPU_ENOSPC round and a second context
on the same index.  The answers are held against the CPU restatements (bytes.find, tests/small_exon_lib.py,
tests/refine_lib.py, tests/chain_lib.py, tests/clean_lib.py, tests/cand_lib.py, tests/fact_lib.py, tests/final_lib.py,
tests/unit_lib.py), never against the library alone; the messages are the literal texts of the source."""
import ctypes as C

import numpy as np
import pytest

import cand_lib as DL
import chain_lib as CL
import clean_lib as KL
import fact_lib as FA
import final_lib as FL
import refine_lib as RL
import small_exon_lib as SL
import unit_lib as UL

pytestmark = pytest.mark.gpu

MESSAGES = {
    "find": "bad find query (reserved != 0, lo > hi, or the pattern leaves the pattern buffer)",
    "small_exons": "bad small-exon query (reserved != 0, min_intron_len < 4, or efact / allgfact leave their sequence)",
    "refine_introns": "bad refine query (an offset past its buffer, an unknown flag, dim == 0, a donor that is not in front of "
                      "the acceptor, or a coordinate outside what it indexes)",
    "refine_chains": "bad chain query (a range past its buffer, reserved != 0, no exon, an exon two chains share, a donor that "
                     "is not in front of its acceptor, or a coordinate outside what it indexes)",
    "clean_chains": "bad clean query (a range past its buffer, an empty EST, reserved != 0, no exon, an exon two queries share, a "
                    "coordinate outside what it indexes, or an end exon that begins in front of or ends behind its sequence)",
    "candidates": "bad candidate parameters (min_factor_len 0 or above 2^24)",
    "factorizations": "bad factorization query (a range past its buffer, an empty EST, reserved != 0, or an exon two queries share)",
    "final_factorizations": "bad final query (a range past its buffer, an empty EST, reserved != 0, or an exon two queries share)",
    "unit_records": "bad unit (flag bits beyond 0-1)",
}


def occurrences(gen, pat, lo, hi):
    hi = min(hi, len(gen))
    out, t = [], gen.find(pat, lo, hi)
    while t >= 0:
        out.append(t)
        t = gen.find(pat, t + 1, hi)
    return out


def find_on(ctx, idx, blob, queries, n, out):
    """pgpu_index_find on any context that shares the index -> (rc, first, n_out)"""
    first = np.full(n + 1, 7, dtype=np.uint64)
    total = C.c_size_t(99)
    rc = ctx.L.pgpu_index_find(ctx.h, idx.h, blob, len(blob), queries, n, out.ctypes.data_as(C.POINTER(C.c_uint32)), len(out),
                               first.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(total))
    return rc, first, total.value


class Entry:
    """one entry on the shared index: good() -> (rc, answer as bytes), bad() and empty() -> rc, ms() -> the slots"""


@pytest.fixture(scope="module")
def world(O):
    import pintron_amd.capi as capi
    rng = np.random.default_rng(12)
    g = bytearray(RL.rnd(rng, 700))
    made = None
    while made is None or made[4] >= 370:              # one chain of two exons in the first half of the sequence
        if made is not None:
            for p, s in reversed(saved):
                g[p:p + len(s)] = s
        before = bytes(g)
        made = CL.make_chain(rng, g, 40, 2, aims=[None])
        if made is not None:
            saved = [(p, before[p:p + len(s)]) for p, s in made[3]]
    est, exons, st = made[:3]
    e1, s0, sl, e2 = 410, 530, 12, 652                  # exon1 GT..AG small exon GT..AG exon2 behind it
    g[e1:e1 + 2], g[s0 - 2:s0], g[s0 + sl:s0 + sl + 2], g[e2 - 2:e2] = b"GT", b"AG", b"GT", b"AG"
    gen = bytes(g)
    ctx = capi.Context(0)                               # its own: the timing switch is turned here
    idx = capi.Index(ctx, gen)
    entries = {}

    # find: three patterns cut from the sequence, in the whole of it and in a window
    pats = [gen[100:106], gen[300:304], b"GT"]
    wins = [(0, 700), (250, 400), (0, 9999)]
    want_pos = [occurrences(gen, p, lo, hi) for p, (lo, hi) in zip(pats, wins)]
    assert all(want_pos) and sum(len(w) for w in want_pos) > 3
    blob = b"".join(pats)

    def find_queries(reserved=0):
        q, off = (capi.FindQuery * len(pats))(), 0
        for i, (p, (lo, hi)) in enumerate(zip(pats, wins)):
            q[i] = capi.FindQuery(off, len(p), reserved if i == 1 else 0, lo, hi)
            off += len(p)
        return q
    total_want, fq = sum(len(w) for w in want_pos), find_queries()

    def find_good():
        out = np.zeros(total_want, dtype=np.uint32)
        rc, first, total = find_on(ctx, idx, blob, fq, len(pats), out)
        return rc, first.tobytes() + out.tobytes()
    want_first = np.cumsum([0] + [len(w) for w in want_pos]).astype(np.uint64)
    e = entries["find"] = Entry()
    e.total, e.blob, e.queries, e.want_pos = total_want, blob, fq, want_pos
    e.good = find_good
    e.want = want_first.tobytes() + np.array(sum(want_pos, []), dtype=np.uint32).tobytes()
    e.bad = lambda: find_on(ctx, idx, blob, find_queries(reserved=1), len(pats), np.zeros(total_want, dtype=np.uint32))[0]
    e.empty = lambda: find_on(ctx, idx, blob, fq, 0, np.zeros(total_want, dtype=np.uint32))[0]
    e.ms = lambda: tuple(idx.find_kernel_ms().values())

    # small exons: the planted one with and without borders, and a factor cut anywhere
    rows = [(gen[e1 - a:e1] + gen[s0:s0 + sl] + gen[e2:e2 + b], e1 - a, e2 + b - (e1 - a), a + 6, b + 6, 40) for a, b in ((4, 3), (0, 0))]
    rows.append((gen[450:470], 380, 300, 8, 8, 4))
    sq = np.zeros(len(rows), dtype=np.dtype(SL.QUERY_DTYPE))
    off = 0
    for i, (ef, gs, gl, f1, f2, mil) in enumerate(rows):
        sq[i] = (off, len(ef), gs, gl, f1, f2, mil, 0, 0)
        off += len(ef)
    sests = b"".join(r[0] for r in rows)
    want_se = SL.transcribe(gen, sests, sq, SL.reference_classify(gen))
    sres = np.zeros(len(rows), dtype=np.dtype(capi.SEXON_RESULT_DTYPE))
    for i, w in enumerate(want_se):
        for f, v in zip(("len", "offstart", "offend", "gpos", "i1type", "i2type"), w):
            sres[i][f] = v
    sbad = sq.copy()
    sbad["min_intron_len"][1] = 3
    e = entries["small_exons"] = Entry()
    e.good = lambda: (lambda rc, res: (rc, res.tobytes()))(*idx.small_exons_raw(sests, sq, len(sq)))
    e.want = sres.tobytes()
    e.bad = lambda: idx.small_exons_raw(sests, sbad, len(sbad))[0]
    e.empty = lambda: idx.small_exons_raw(sests, sq, 0)[0]
    e.ms = lambda: (idx.small_exons_kernel_ms(),)

    # refine_introns: the chain's intron as the first and as a later one, rows from the oracle's CPU gap alignment
    er, gr, v = RL.oracle_rows(O, est, gen, exons[0], exons[1], *st[:3])
    items = [(est, er, gr, v, exons[0], exons[1], first, st) for first in (True, False)]
    rests, rrows, rq = RL.query_array(items)
    want_r = [RL.refine(est, gen, er, gr, v, exons[0], exons[1], first, *st) for first in (True, False)]
    assert all(w[0] == RL.OK for w in want_r)
    rres = np.zeros(len(items), dtype=np.dtype(capi.REFINE_RESULT_DTYPE))
    for i, (status, refined, path, d, a) in enumerate(want_r):
        rres[i] = (status, refined, path, 0, d, a)
    rbad = rq.copy()
    rbad["dim"][1] = 0
    e = entries["refine_introns"] = Entry()
    e.good = lambda: (lambda rc, res: (rc, res.tobytes()))(*idx.refine_introns_raw(rests, rrows, rq, len(rq)))
    e.want = rres.tobytes()
    e.bad = lambda: idx.refine_introns_raw(rests, rrows, rbad, len(rbad))[0]
    e.empty = lambda: idx.refine_introns_raw(rests, rrows, rq, 0)[0]
    e.ms = lambda: (idx.refine_introns_kernel_ms(),)

    # refine_chains: the chain under its settings and with min_intron_length 4
    batch = [(est, exons, st), (est, exons, st[:3] + (4,))]
    cests, cexons, cq = CL.batch_arrays(batch)
    want_c = [CL.chain(x, gen, ex, s) for x, ex, s in batch]
    assert all(w[0] == CL.OK for w in want_c)
    oex, ost = cexons.copy(), np.zeros(len(cexons), dtype=np.uint8)
    cres = np.zeros(len(batch), dtype=np.dtype(capi.CHAIN_RESULT_DTYPE))
    k = 0
    for i, (status, done, dropped, ex2, steps) in enumerate(want_c):
        cres[i] = (status, done, dropped, 0)
        for x, s in zip(ex2, steps):
            oex[k], ost[k] = tuple(x), s
            k += 1
    cbad = cq.copy()
    cbad["reserved"][1] = 1

    def chains(q, n):
        rc, a, b, c = idx.refine_chains_raw(cests, cexons, q, n)
        return rc, a.tobytes() + b.tobytes() + c.tobytes()
    e = entries["refine_chains"] = Entry()
    e.good = lambda: chains(cq, len(cq))
    e.want = oex.tobytes() + ost.tobytes() + cres.tobytes()
    e.bad = lambda: chains(cbad, len(cbad))[0]
    e.empty = lambda: chains(cq, 0)[0]
    e.empty_answer = cexons.tobytes() + bytes(len(cexons))          # n == 0: the exons copied, the steps zeroed
    e.chains = chains
    e.cq = cq
    e.ms = lambda: (idx.refine_chains_kernel_ms(),)

    # clean_chains: the chain's two exons twice, under the complexity thresholds 20.0 and 0.32.  (The restatement takes
    # them past step 1 and within every cap: both queries end at the coverage check, with different marks on the way.)
    kbatch = [(est, exons, 20.0), (est, exons, 0.32)]
    kests, kexons, kq = KL.batch_arrays(kbatch)
    want_k = [KL.clean(x, gen, ex, thr) for x, ex, thr in kbatch]
    assert all(w[0] == KL.OK and w[1] not in (1, 2) for w in want_k) and want_k[0][5] != want_k[1][5]
    kbad = kq.copy()
    kbad["reserved"][1] = 1

    def cleaned(q, n, marks_fill=0):
        """as capi's clean_chains_raw, with out_marks filled beforehand"""
        oe, om = np.zeros_like(kexons), np.full(len(kexons), marks_fill, dtype=np.uint8)
        res = np.zeros(n, dtype=np.dtype(capi.CLEAN_RESULT_DTYPE))
        rc = ctx.L.pgpu_index_clean_chains(ctx.h, idx.h, kests, len(kests), kexons.ctypes.data_as(C.POINTER(capi.Factor)), len(kexons),
                                           q.ctypes.data_as(C.POINTER(capi.CleanQuery)), n, oe.ctypes.data_as(C.POINTER(capi.Factor)),
                                           om.ctypes.data_as(C.POINTER(C.c_uint8)), res.ctypes.data_as(C.POINTER(capi.CleanResult)))
        return rc, oe.tobytes() + om.tobytes() + res.tobytes()
    e = entries["clean_chains"] = Entry()
    e.good = lambda: cleaned(kq, len(kq))
    e.want = b"".join(a.tobytes() for a in KL.expect_arrays(kexons, want_k))
    e.bad = lambda: cleaned(kbad, len(kbad))[0]
    e.empty = lambda: cleaned(kq, 0)[0]
    e.empty_answer = kexons.tobytes() + bytes(len(kexons))          # n == 0: the exons copied, the marks zeroed
    e.cleaned = cleaned
    e.kq = kq
    e.ms = lambda: (idx.clean_chains_kernel_ms(),)

    # ---- the index forms of the four device stages, two queries each: the chain's two exons, and a single short exon (the
    # first thirty bases of the chain's first one).  Every kernel of a stage runs once; in the factorizations the chain ends
    # EMPTY at the cleaning and the short exon is DONE, so the compact answer has one exon and is copied out.
    chain_ex = [tuple(int(v) for v in x) for x in exons]
    short_ex = [(chain_ex[0][0], chain_ex[0][0] + 29, chain_ex[0][2], chain_ex[0][2] + 29)]
    lo = chain_ex[0][0]
    est2, est1 = est[lo:chain_ex[-1][1] + 1], est[lo:lo + 30]            # the stretches of the EST the two lists cover
    chain2, short1 = [(a - lo, b - lo, g0, g1) for a, b, g0, g1 in chain_ex], [(0, 29) + short_ex[0][2:]]

    # candidates: one record per list, a pairing per exon
    recs = [DL.record(*DL.chain([(a, g0, min(b - a, g1 - g0) + 1) for a, b, g0, g1 in ex])) for ex in (chain_ex, short_ex)]
    dblob, dfirst = DL.batch(recs)
    dres, dex = DL.expect_arrays([DL.candidate(r, gen, 15, 40) for r in recs])

    def candidates(n, L=15):
        rc, res, ex, total = idx.candidates_raw(dblob, dfirst, n, L, 40, len(dex))
        return rc, res.tobytes() + ex[:total].tobytes()
    e = entries["candidates"] = Entry()
    e.good = lambda: candidates(len(recs))
    e.want = dres.tobytes() + dex.tobytes()
    e.bad = lambda: candidates(len(recs), L=0)[0]
    e.empty = lambda: candidates(0)[0]
    e.ms = lambda: (idx.candidates_kernel_ms(),)

    # factorizations
    aests, aexons, aq = FA.batch_arrays([(est2, chain2), (est1, short1)])
    awant = FA.expect_arrays([FA.factorization(DL.ONE, x, gen, ex) for x, ex in ((est2, chain2), (est1, short1))])
    assert [int(o) for o in awant[0]["outcome"]] == [FA.EMPTY, FA.DONE] and len(awant[1]) == 1
    abad = aq.copy()
    abad["reserved"][1] = 1

    def factorizations(q, n):
        rc, res, ex, st, total = idx.factorizations_raw(aests, aexons, q, n, capi.FactParams(*FA.DEFAULTS), len(aexons))
        return rc, res.tobytes() + ex[:total].tobytes() + st[:total].tobytes()
    e = entries["factorizations"] = Entry()
    e.good = lambda: factorizations(aq, len(aq))
    e.want = b"".join(a.tobytes() for a in awant)
    e.bad = lambda: factorizations(abad, len(abad))[0]
    e.empty = lambda: factorizations(aq, 0)[0]
    e.ms = lambda: (idx.factorizations_kernel_ms(),)

    # final factorizations: the ESTs are their own originals
    nests, nexons, nq = FL.batch_arrays([(est2, est2, chain2), (est1, est1, short1)])
    nwant = FL.expect_arrays([FL.final(DL.ONE, x, x, gen, ex, FA.DEFAULTS, 40) for x, ex in ((est2, chain2), (est1, short1))])
    assert [int(o) for o in nwant[0]["outcome"]] == [FL.EMPTY, FL.DONE] and len(nwant[1]) == 1
    nbad = nq.copy()
    nbad["reserved"][1] = 1

    def finals(q, n):
        rc, res, ex, st, total = idx.final_factorizations_raw(nests, nexons, q, n, capi.FactParams(*FA.DEFAULTS), capi.SmallParams(40, 0),
                                                              2 * len(nexons))
        return rc, res.tobytes() + ex[:total].tobytes() + st[:total].tobytes()
    e = entries["final_factorizations"] = Entry()
    e.good = lambda: finals(nq, len(nq))
    e.want = b"".join(a.tobytes() for a in nwant)
    e.bad = lambda: finals(nbad, len(nbad))[0]
    e.empty = lambda: finals(nq, 0)[0]
    e.ms = lambda: (idx.final_factorizations_kernel_ms(),)

    # unit records: an aligned pattern with its sibling, and one whose only pattern has a single short exon
    ures, uexons, uempty, uq = UL.batch([dict(fwd=UL.aligned(), rev=UL.aligned((31, 32, 33, 34)), flags=0, est_index=7),
                                         dict(fwd=UL.aligned((2,)), rev=None, flags=0, est_index=9)])
    uout, ublob = UL.units(ures, uexons, uempty, uq)
    ubad = uq.copy()
    ubad["flags"][1] = 4

    def units(q, n):
        rc, out, blob, total = capi.unit_records_raw(ctx, ures, uexons, uempty, q, n, capi.unit_params(0, 1), len(ublob))
        return rc, out.tobytes() + blob[:total].tobytes()
    e = entries["unit_records"] = Entry()
    e.good = lambda: units(uq, len(uq))
    e.want = uout.tobytes() + ublob
    e.bad = lambda: units(ubad, len(ubad))[0]
    e.empty = lambda: units(uq, 0)[0]
    e.ms = lambda: (ctx.L.pgpu_unit_records_kernel_ms(),)

    yield capi, ctx, idx, gen, entries
    idx.close()
    ctx.close()


@pytest.mark.parametrize("name", ["find", "small_exons", "refine_introns", "refine_chains", "clean_chains", "candidates",
                                  "factorizations", "final_factorizations", "unit_records"])
def test_the_contract_of_a_timed_entry(world, name):
    capi, ctx, idx, gen, entries = world
    e = entries[name]
    rc, timed = e.good()
    assert rc == capi.PGPU_OK and timed == e.want                # the CPU restatement's answer
    assert all(ms > 0.0 for ms in e.ms()), e.ms()
    ctx.L.pgpu_set_timing(ctx.h, 0)
    try:
        rc, untimed = e.good()
        assert rc == capi.PGPU_OK and all(ms == 0.0 for ms in e.ms()), e.ms()
        assert untimed == timed
    finally:
        ctx.L.pgpu_set_timing(ctx.h, 1)
    assert e.good()[0] == capi.PGPU_OK and all(ms > 0.0 for ms in e.ms())     # a slot the refusal has to reset
    assert e.bad() == capi.PGPU_EINVAL
    assert all(ms == 0.0 for ms in e.ms()), e.ms()
    assert ctx.L.pgpu_last_error(ctx.h).decode() == MESSAGES[name]
    rc, again = e.good()
    assert rc == capi.PGPU_OK and again == timed and all(ms > 0.0 for ms in e.ms())
    assert e.empty() == capi.PGPU_OK
    assert all(ms == 0.0 for ms in e.ms()), e.ms()


def test_an_empty_chain_call_copies_the_exons(world):
    capi, ctx, idx, gen, entries = world
    e = entries["refine_chains"]
    rc, answer = e.chains(e.cq, 0)
    assert rc == capi.PGPU_OK and answer == e.empty_answer


def test_an_empty_clean_call_copies_the_exons_and_zeroes_the_marks(world):
    capi, ctx, idx, gen, entries = world
    e = entries["clean_chains"]
    rc, answer = e.cleaned(e.kq, 0, marks_fill=0xA5)
    assert rc == capi.PGPU_OK and answer == e.empty_answer


def test_find_without_room_then_with_it_then_on_a_second_context(world):
    capi, ctx, idx, gen, entries = world
    e = entries["find"]
    n, flat = len(e.want_pos), sum(e.want_pos, [])
    short = np.full(e.total - 1, 0xDEADBEEF, dtype=np.uint32)
    rc, first, total = find_on(ctx, idx, e.blob, e.queries, n, short)
    assert rc == capi.PGPU_ENOSPC and total == e.total and int(first[n]) == e.total
    assert ctx.L.pgpu_last_error(ctx.h).decode() == "position buffer too small"
    assert (short == 0xDEADBEEF).all()
    ms = idx.find_kernel_ms()
    assert ms["count+scan"] > 0.0 and ms["fill"] == 0.0          # the first phase ran and was timed, the second did not run
    out = np.zeros(e.total, dtype=np.uint32)
    rc, first, total = find_on(ctx, idx, e.blob, e.queries, n, out)
    assert rc == capi.PGPU_OK and total == e.total and out.tolist() == flat
    assert all(v > 0.0 for v in idx.find_kernel_ms().values())
    with capi.Context(0) as other:
        out2 = np.zeros(e.total, dtype=np.uint32)
        rc, first2, total2 = find_on(other, idx, e.blob, e.queries, n, out2)
        assert rc == capi.PGPU_OK and total2 == e.total and out2.tolist() == flat and np.array_equal(first2, first)
