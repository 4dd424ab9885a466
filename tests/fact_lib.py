"""CPU restatement of the factorization stage (pgpu_pairing_plan_run_factorizations, pgpu_index_factorizations): a
candidate through the cleaning steps, check_gap_errors and the refinement loop, with the glue between them written as
get_EST_factorizations (src/est-factorizations.c) does it -- a list that shrinks, front to back: the kept run of clean, the
exons gaps merged removed, the first exon dropped.

factorization   cand_lib.candidate's answer -> clean_lib.clean -> gaps_lib.gaps -> chain_lib.chain; what a chained
                entry's validator refuses for a whole call (the einval of each library, on the one query) is HOST with
                detail 2 for this EST alone.
expect_arrays   answers -> the three arrays of the entry (results, exons and step bytes, compact, in EST order).
batch_arrays    cases of (est, exons or None) -> (ests, exons array, queries array).
call_by_call    the same answers from the three EXISTING public entries called one after the other (clean_chains,
                gap_chains, refine_chains) with the glue in Python: what a caller had to do before this stage.
hand_cases      what no fixture reaches: HOST at the stages 1-3, and the caps' last accepted values beside each.
"""
import numpy as np

import cand_lib as KL
import chain_lib as RC
import clean_lib as CL
import gaps_lib as GL

HOST, EMPTY, DONE = 0, 1, 2
OK = 0
MERGED = 0x80
DEFAULTS = (20.0, 30, 70, 30, 40)        # complexity_threshold, suffpref on_est / for_intron / on_gen, min_intron_length
FIXTURE_SETTINGS = (30, 30, 30, 60)      # the refine settings the clean and gaps fixtures are pushed through with


def answer(outcome, stage, detail, exons=(), steps=(), n_merged=0, total_edit=0):
    return dict(outcome=outcome, stage=stage, detail=detail, exons=[tuple(e) for e in exons], steps=list(steps),
                n_merged=n_merged, total_edit=total_edit)


def _one_query(est, n):
    return [dict(est_off=0, est_len=len(est), first_exon=0, n_exons=n, reserved=0)]


def factorization(kind, est: bytes, gen: bytes, exons, prm=DEFAULTS, info=None):
    """One EST -> answer().  kind: cand_lib's (ONE goes down the chain); exons: the candidate's, [(EST_start, EST_end,
    GEN_start, GEN_end)]; prm = (complexity_threshold, suffpref_length_on_est, _for_intron, _on_gen, min_intron_length).
    `info` (a dict) receives "est_gap" (the list gaps saw had an unaligned EST gap) and the three stage answers."""
    info = {} if info is None else info
    thr, settings = prm[0], tuple(prm[1:])
    if kind in (KL.NONE, KL.NOT_PATH):
        return answer(HOST, 0, kind)
    if kind == KL.REFUSED:
        return answer(EMPTY, 0, KL.REFUSED)
    lst = [tuple(int(v) for v in e) for e in exons]
    # ---- clean (:212-244)
    if CL.einval(len(est), len(gen), lst, _one_query(est, len(lst))):
        return answer(HOST, 1, 2)
    status, verdict, first, n, after, marks = info["clean"] = CL.clean(est, gen, lst, thr)
    if status != OK:
        return answer(HOST, 1, 1)
    if verdict != 0:
        return answer(EMPTY, 1, verdict)
    lst = after[first:first + n]                                      # the kept run
    # ---- check_gap_errors (:416-433)
    if GL.einval(len(est), len(gen), lst, _one_query(est, len(lst))):
        return answer(HOST, 2, 2)
    info["est_gap"] = RC.has_est_gap(lst)
    status, verdict, total, kept, after, steps = info["gaps"] = GL.gaps(est, gen, lst)
    if status != OK:
        return answer(HOST, 2, 1)
    if verdict != 0:
        return answer(EMPTY, 2, 1, total_edit=total)
    lst = [e for e, s in zip(after, steps) if not s & MERGED]         # the merged exons removed
    n_merged = len(after) - len(lst)
    assert len(lst) == kept
    # ---- the refinement loop (:446-490)
    if any(d[1] >= a[0] or d[3] >= a[2] for d, a in zip(lst, lst[1:])):
        return answer(HOST, 3, 2, total_edit=total)
    status, done, dropped, after, steps = info["refine"] = RC.chain(est, gen, lst, settings)
    if status != OK:
        return answer(HOST, 3, 1, total_edit=total)
    if dropped:                                                       # the first-exon rule (:476-485)
        after, steps = after[1:], steps[1:]
    return answer(DONE, 3, dropped, after, steps, n_merged, total)


def expect_arrays(answers):
    """answers of factorization() per EST -> (results, exons, steps) as the entry writes them"""
    from pintron_amd import capi
    res = np.zeros(len(answers), dtype=np.dtype(capi.FACT_RESULT_DTYPE))
    ex, st = [], []
    for i, a in enumerate(answers):
        done = a["outcome"] == DONE
        res[i] = (a["outcome"], a["stage"], a["detail"], len(ex) if done else 0, len(a["exons"]) if done else 0,
                  a["n_merged"] if done else 0, a["total_edit"])
        if done:
            ex += a["exons"]
            st += a["steps"]
    return res, np.array(ex, dtype=np.dtype(capi.FACTOR_DTYPE)).reshape(-1), np.array(st, dtype=np.uint8)


def batch_arrays(cases):
    """cases of (est, exons) -- exons None or empty: no candidate -> (ests, exons array, queries array); equal ESTs are stored
    once"""
    from pintron_amd import capi
    n_ex = sum(len(c[1] or ()) for c in cases)
    exons = np.zeros(n_ex, dtype=np.dtype(capi.FACTOR_DTYPE))
    q = np.zeros(len(cases), dtype=np.dtype(capi.FACT_QUERY_DTYPE))
    ests, eat, eoff, k = [], {}, 0, 0
    for i, (est, ex) in enumerate(cases):
        ex = ex or ()
        if est not in eat:
            eat[est] = eoff
            ests.append(est)
            eoff += len(est)
        for e in ex:
            exons[k] = tuple(e)
            k += 1
        q[i] = (eat[est], len(est), k - len(ex) if ex else 0, len(ex), 0)
    return b"".join(ests), exons, q


def plan_queries(pat_off, cand_res):
    """the queries of the index form that name the candidates a plan fetched (REFUSED, NONE and NOT_PATH: no candidate)"""
    from pintron_amd import capi
    q = np.zeros(len(cand_res), dtype=np.dtype(capi.FACT_QUERY_DTYPE))
    q["est_off"] = pat_off[:-1]
    q["est_len"] = np.diff(pat_off)
    one = cand_res["kind"] == KL.ONE
    q["first_exon"] = np.where(one, cand_res["first_exon"], 0)
    q["n_exons"] = np.where(one, cand_res["n_exons"], 0)
    return q


def stage0_of_kinds(res, kinds):
    """results of the index form (every EST without a candidate: HOST, detail NONE) -> what the plan form says of the same
    ESTs, which knows the candidate's kind"""
    res = res.copy()
    for i in np.nonzero(kinds != KL.ONE)[0]:
        k = int(kinds[i])
        res[i] = (EMPTY if k == KL.REFUSED else HOST, 0, k, 0, 0, 0, 0)
    return res


# ---- the call-by-call route: the three public entries one after the other, the glue on the host ----------------------
def _sub_batch(ests, exons, queries, live, ranges, dtype, extra=()):
    """the queries `live` over the exon ranges `ranges` {i: (first, n)} of `exons`, as a call of their own"""
    n_ex = sum(ranges[i][1] for i in live)
    ex = np.zeros(n_ex, dtype=exons.dtype)
    q = np.zeros(len(live), dtype=np.dtype(dtype))
    k = 0
    for j, i in enumerate(live):
        first, n = ranges[i]
        ex[k:k + n] = exons[first:first + n]
        q[j] = (int(queries["est_off"][i]), int(queries["est_len"][i]), k, n, 0) + tuple(extra)
        k += n
    return ex, q


def _tuples(arr):
    return [tuple(int(v) for v in e) for e in arr]


def call_by_call(idx, gen_len, ests: bytes, exons, queries, prm=DEFAULTS, clock=None):
    """The arrays of expect_arrays from pgpu_index_clean_chains, pgpu_index_gap_chains and pgpu_index_refine_chains called
    one after the other.  Between them the host does what the stage does on the device; what an entry would refuse for the
    whole call is taken out of its batch beforehand (HOST, detail 2).  `clock` (a dict) receives "kernel_ms", the three kernel times, and "library_s", the
    seconds inside the three entries."""
    import time
    from pintron_amd import capi
    inside = 0.0
    thr, settings = prm[0], tuple(prm[1:])
    n = len(queries)
    out = [None] * n
    total_edit = [0] * n
    one = lambda i, k: [dict(est_off=0, est_len=int(queries["est_len"][i]), first_exon=0, n_exons=k, reserved=0)]
    # stage 0 and clean's rules
    ranges, live = {}, []
    for i in range(n):
        ne = int(queries["n_exons"][i])
        if ne == 0:
            out[i] = answer(HOST, 0, KL.NONE)
            continue
        first = int(queries["first_exon"][i])
        if CL.einval(int(queries["est_len"][i]), gen_len, _tuples(exons[first:first + ne]), one(i, ne)):
            out[i] = answer(HOST, 1, 2)
            continue
        ranges[i] = (first, ne)
        live.append(i)
    ms = [0.0, 0.0, 0.0]
    kept = {}
    if live:
        ex, q = _sub_batch(ests, exons, queries, live, ranges, capi.CLEAN_QUERY_DTYPE, (thr,))
        t0 = time.perf_counter()
        ex2, _, res = idx.clean_chains(ests, ex, q)
        inside += time.perf_counter() - t0
        ms[0] = idx.clean_chains_kernel_ms()
        nxt = []
        for j, i in enumerate(live):
            if res["status"][j] != OK:
                out[i] = answer(HOST, 1, 1)
            elif res["verdict"][j] != 0:
                out[i] = answer(EMPTY, 1, int(res["verdict"][j]))
            else:
                at = int(q["first_exon"][j]) + int(res["first_kept"][j])
                lst = _tuples(ex2[at:at + int(res["n_kept"][j])])
                if GL.einval(int(queries["est_len"][i]), gen_len, lst, one(i, len(lst))):
                    out[i] = answer(HOST, 2, 2)
                else:
                    kept[i] = lst
                    nxt.append(i)
        live = nxt
    if live:
        flat = np.array([e for i in live for e in kept[i]], dtype=exons.dtype).reshape(-1)
        ranges, k = {}, 0
        for i in live:
            ranges[i] = (k, len(kept[i]))
            k += len(kept[i])
        ex, q = _sub_batch(ests, flat, queries, live, ranges, capi.GAPS_QUERY_DTYPE)
        t0 = time.perf_counter()
        ex2, steps, res = idx.gap_chains(ests, ex, q)
        inside += time.perf_counter() - t0
        ms[1] = idx.gap_chains_kernel_ms()
        nxt, merged = [], {}
        for j, i in enumerate(live):
            if res["status"][j] != OK:
                out[i] = answer(HOST, 2, 1)
                continue
            total_edit[i] = int(res["total_edit"][j])
            if res["verdict"][j] != 0:
                out[i] = answer(EMPTY, 2, 1, total_edit=total_edit[i])
                continue
            first, ne = int(q["first_exon"][j]), int(q["n_exons"][j])
            lst = [e for e, s in zip(_tuples(ex2[first:first + ne]), steps[first:first + ne]) if not s & MERGED]
            merged[i] = ne - len(lst)
            if any(d[1] >= a[0] or d[3] >= a[2] for d, a in zip(lst, lst[1:])):
                out[i] = answer(HOST, 3, 2, total_edit=total_edit[i])
            else:
                kept[i] = lst
                nxt.append(i)
        live = nxt
    if live:
        flat = np.array([e for i in live for e in kept[i]], dtype=exons.dtype).reshape(-1)
        ranges, k = {}, 0
        for i in live:
            ranges[i] = (k, len(kept[i]))
            k += len(kept[i])
        ex, q = _sub_batch(ests, flat, queries, live, ranges, capi.CHAIN_QUERY_DTYPE, settings)
        t0 = time.perf_counter()
        ex2, steps, res = idx.refine_chains(ests, ex, q)
        inside += time.perf_counter() - t0
        ms[2] = idx.refine_chains_kernel_ms()
        for j, i in enumerate(live):
            if res["status"][j] != OK:
                out[i] = answer(HOST, 3, 1, total_edit=total_edit[i])
                continue
            first, ne, dropped = int(q["first_exon"][j]), int(q["n_exons"][j]), int(res["dropped_first"][j])
            out[i] = answer(DONE, 3, dropped, _tuples(ex2[first + dropped:first + ne]), [int(s) for s in steps[first + dropped:first + ne]],
                            merged[i], total_edit[i])
    if clock is not None:
        clock["kernel_ms"], clock["library_s"] = ms, inside
    return expect_arrays(out)


# ---- the fixtures of the three chained entries, as candidates -------------------------------------------------------
_fixtures = {}


def fixture_groups(name):
    """(genomic, {prm: [(est, exons)]}) of one of the three committed fixtures ("clean_chains", "gap_chains",
    "refine_chains"), grouped by the parameters of a call.  Shared: do not modify."""
    if name not in _fixtures:
        groups = {}
        if name == "clean_chains":
            gen, cases = CL.load_fixture()
            for c in cases:
                groups.setdefault((c["thr"],) + FIXTURE_SETTINGS, []).append((c["est"], c["exons"]))
        elif name == "gap_chains":
            gen, cases = GL.load_fixture()
            groups[(20.0,) + FIXTURE_SETTINGS] = [(c["est"], c["exons"]) for c in cases]
        else:
            gen, cases = RC.load_fixture()
            for c in cases:
                groups.setdefault((20.0,) + tuple(c["settings"]), []).append((c["est"], c["exons"]))
        _fixtures[name] = (gen, groups)
    return _fixtures[name]


_answers = {}


def _restate(name):
    if name not in _answers:
        gen, groups = fixture_groups(name)
        ans, infos = {}, {}
        for prm, cases in groups.items():
            infos[prm] = [{} for _ in cases]
            ans[prm] = [factorization(KL.ONE, est, gen, ex, prm, info) for (est, ex), info in zip(cases, infos[prm])]
        _answers[name] = (ans, infos)
    return _answers[name]


def fixture_answers(name):
    """{prm: [answer]} of fixture_groups(name), by the restatement; computed once.  Shared: do not modify."""
    return _restate(name)[0]


def fixture_infos(name):
    """{prm: [info]}: what factorization() noted of the same cases (the three stage answers among it)"""
    return _restate(name)[1]


# ---- hand-made cases: HOST at the stages 1-3, the caps' last accepted values beside each ------------------------------
HAND_LEN = 30_000


def hand_sequence():
    rng = np.random.default_rng(4711)
    return bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, HAND_LEN)])


def _exons(gen, lens, introns, at=1000, est_gaps=None, gen_extra=None):
    """an EST of exons copied from `gen` (lens), separated there by `introns`; est_gaps[k]: bytes of the EST between exon k
    and k + 1 that belong to no exon (random; the genomic gap is the intron).  -> (est, exons)"""
    rng = np.random.default_rng(len(lens) * 131 + at)
    est, exons, g = bytearray(b"ACGTTGCAAC"), [], at
    for k, n in enumerate(lens):
        exons.append((len(est), len(est) + n - 1, g, g + n - 1))
        est += gen[g:g + n]
        g += n + (introns[k] if k < len(introns) else 0)
        if est_gaps and k < len(lens) - 1 and est_gaps[k]:
            gp = est_gaps[k]
            if gp <= introns[k]:                       # the two ends of the intron: the border refinement finds them
                est += gen[g - introns[k]:g - introns[k] + gp // 2] + gen[g - (gp - gp // 2):g]
            else:
                est += bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, gp)])
    est += b"TTGACCA"
    return bytes(est), exons


def hand_cases():
    """[(name, est, exons or None, prm, (outcome, stage, detail) expected or None)] over hand_sequence()"""
    g = hand_sequence()
    out = []
    D = DEFAULTS

    def add(name, est, exons, want, prm=D):
        out.append((name, est, exons, prm, want))

    plain = _exons(g, [80, 90, 100], [300, 400])
    add("plain", *plain, (DONE, 3, None))
    add("no_candidate", plain[0], None, (HOST, 0, KL.NONE))
    # clean's caps: 64 exons pass, 65 are refused; an end exon of 4 096 bytes passes, 4 097 is refused
    add("exons_64", *_exons(g, [40] * 64, [120] * 63), (DONE, 3, None))
    add("exons_65", *_exons(g, [40] * 65, [120] * 64), (HOST, 1, 1))
    # (an exon of more than 1 033 genomic bytes meets another cap at step 5: under a threshold every exon fails, step 4
    # empties the list first, and the cap of step 2 alone decides between the two)
    add("end_exon_4096", *_exons(g, [4096, 90], [300], at=2000), (EMPTY, 1, 5), (0.01,) + D[1:])
    add("end_exon_4097", *_exons(g, [4097, 90], [300], at=2000), (HOST, 1, 1), (0.01,) + D[1:])
    # clean's validator: a coordinate outside factor_ok; an end exon that ends behind its EST
    est, ex = plain
    add("coordinate_outside", est, [ex[0], (ex[1][0], len(est) + 1, ex[1][2], ex[1][3]), ex[2]], (HOST, 1, 2))
    add("coordinate_at_length", est, [ex[0], ex[1], (ex[2][0], len(est), ex[2][2], ex[2][3])], (HOST, 1, 2))
    add("genomic_outside", est, [ex[0], ex[1], (ex[2][0], ex[2][1], HAND_LEN + 1, HAND_LEN + 2)], (HOST, 1, 2))
    # gaps' cap: an EST gap of 64 behind a clean pass, and of 65
    add("est_gap_64", *_exons(g, [80, 90, 100], [300, 400], at=8000, est_gaps=[64, 0]), None)
    add("est_gap_65", *_exons(g, [80, 90, 100], [300, 400], at=8000, est_gaps=[65, 0]), (HOST, 2, 1))
    # gaps' validator: gapP > gapT (an EST gap of 30 over a genomic gap of 20), and gapP == gapT beside it
    add("gap_p_above_gap_t", *_exons(g, [80, 90, 100], [20, 400], at=9000, est_gaps=[30, 0]), (HOST, 2, 2))
    add("gap_p_equals_gap_t", *_exons(g, [80, 90, 100], [30, 400], at=9000, est_gaps=[30, 0]), None)
    # ... and exons that touch on the EST in the wrong order (step 1 of clean tests start < previous end only)
    add("exons_overlap_by_one", est, [ex[0], (ex[0][1], ex[1][1], ex[1][2], ex[1][3]), ex[2]], (HOST, 2, 2))
    # refine's caps need other settings than the defaults.  The middle exon has 96 bytes, so a suffpref length of 97 takes
    # 97 bytes of the first exon and 96 of the middle one: an EST window of 192 passes (96 + 96) and 193 does not; a
    # genomic window of 320 (96 + 64 + 64 + 96) and of 321
    wide = _exons(g, [200, 96, 200], [600, 700], at=12000)
    add("est_window_192", *wide, (DONE, 3, None), (20.0, 96, 30, 30, 40))
    add("est_window_193", *wide, (HOST, 3, 1), (20.0, 97, 30, 30, 40))
    add("gen_window_320", *wide, (DONE, 3, None), (20.0, 30, 64, 96, 40))
    add("gen_window_321", *wide, (HOST, 3, 1), (20.0, 30, 64, 97, 40))
    return g, out
