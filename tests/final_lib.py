"""CPU restatement of the final stage (pgpu_pairing_plan_run_final_factorizations, pgpu_index_final_factorizations): the
factorization stage's restatement, then the tail stage's and the small stage's, with the glue between them as
get_EST_factorizations and refine_EST_factorizations have it -- the exons step 5 of tail removed taken out, the kept run
of small's list cut out.

final           fact_lib.factorization -> tail_lib.tail -> small_lib.small; what a chained entry's validator refuses for a
                whole call (the einval of each library, on the one query) is HOST with detail 2 for this EST alone.  Three
                arguments break the glue on purpose (the cases must notice): tail on the working sequence, small's step 3
                on the working sequence, the removed exons left in.
expect_arrays   answers -> the three arrays of the entry (results, exons and step bytes, compact, in EST order).
batch_arrays    cases of (orig, est, exons or None) -> (ests, exons array, queries array).
route           the same answers from the EXISTING public entries called one after the other (pgpu_index_factorizations,
                pgpu_index_tail_chains, pgpu_index_small_chains) with the glue in Python: what a caller has to do today.
tags_of         what a case reached.
hand_groups     hand-made cases as candidates, over the seeded sequences of the tail and the small fixture, of fact_lib's
                hand-made cases and of own_world (what the fixtures' cases do not bring through the stages 0-3): their
                exons are copies of the sequence, so most pass those stages as they are; the restatement says which, and
                only what arrives counts.  NOT_REACHED names the tags of the cover that nothing reaches, and why.
"""
import numpy as np

import cand_lib as KL
import fact_lib as F
import small_lib as SL
import tail_lib as TL

HOST, EMPTY, DONE = F.HOST, F.EMPTY, F.DONE
OK = 0
FIELDS = ("outcome", "stage", "detail", "n_merged", "total_edit", "tail_added", "polyA", "polyadenil", "recovered", "refused",
          "n_removed", "n_added", "n_cleaned", "prefix_added")

# what the cases the GPU tests use must reach, MIN_PER_TAG times each (tests/test_final_cpu.py)
TAGS = ("done_plain",
        "tail_affix_256", "tail_affix_257", "tail_window_128", "tail_window_129", "tail_gen_256", "tail_gen_257",
        "tail_exons_64", "tail_exons_65",
        "small_refused_1", "small_refused_2", "small_refused_3", "small_refused_4", "small_refused_5",
        "small_window_256", "small_window_257", "small_kband_31", "small_kband_32",
        "empty_4", "empty_5_noisy", "empty_5_external",
        "prefix_exon", "between_exon", "grow_past_64", "removed_reanalysed",
        "polyA", "polyadenil", "recovered_prefix", "recovered_suffix", "tail_added",
        "orig_decides", "host_4_validator")
MIN_PER_TAG = 3
# ... of which nine cannot arrive through the stages 0-3.  The branches of the hand-off kernels that
# carry them are run over stage results made by hand (probe_cases, pgpu_final_handoffs_probe), MIN_PER_TAG cases each:
#   tail_exons_65, small_refused_1   clean refuses a 65th exon, and no stage before small adds one
#   tail_window_128 / _129           check_gap_errors leaves no EST gap, so a window is at most 5 + 100 + 5 bytes
#   tail_gen_256 / _257              an exon of at most 100 EST bytes over 256 genomic ones is noisy for clean's step 5
#   empty_4, small_refused_5         what gaps keeps is strictly ordered, refine moves a border inside its two exons, step 1
#                                    of tail only lengthens the last exon, and no case was found in which step 5 of tail
#                                    merges with off_t1 > off_t2
#   host_4_validator                 clean's validator wants the end exons inside their strings and its step 1 the others
#                                    between them: no coordinate equal to a length gets as far as refine
NOT_REACHED = ("tail_exons_65", "small_refused_1", "tail_window_128", "tail_window_129", "tail_gen_256", "tail_gen_257",
               "empty_4", "small_refused_5", "host_4_validator")


def _one_query(est, n):
    return [dict(est_off=0, est_len=len(est), first_exon=0, n_exons=n, reserved=0, orig_off=0)]


def final(kind, orig: bytes, est: bytes, gen: bytes, exons, prm=F.DEFAULTS, mil=None, ops=None, info=None,
          tail_on_working=False, clean_on_working=False, keep_removed=False):
    """One EST -> a dict of FIELDS, "exons" and "steps".  kind, exons, prm: as fact_lib.factorization, which runs on the
    working sequence `est`; mil: the small stage's min_intron_length (None: prm's).  `info` (a dict) receives "fact", "tail"
    and "small", the three libraries' infos, and the answers "tail_answer" and "small_answer"."""
    info = {} if info is None else info
    mil = int(prm[4]) if mil is None else mil
    fi, ti, si = info.setdefault("fact", {}), info.setdefault("tail", {}), info.setdefault("small", {})
    a = F.factorization(kind, est, gen, exons, prm, fi)
    out = dict.fromkeys(FIELDS, 0)
    out.update(outcome=a["outcome"], stage=a["stage"], detail=a["detail"], n_merged=a["n_merged"], total_edit=a["total_edit"],
               exons=[], steps=[])
    if a["outcome"] != DONE:
        out["n_merged"] = 0
        return out
    dropped = a["detail"] & 1

    def settle(outcome, stage, detail):
        out.update(outcome=outcome, stage=stage, detail=detail)
        return out
    # ---- tail (get_EST_factorizations :573-585, refine_EST_factorizations :1270-1290)
    lst = a["exons"]
    if TL.einval(len(est), len(gen), lst, _one_query(est, len(lst))):
        return settle(HOST, 4, 2)
    t = info["tail_answer"] = TL.tail(est if tail_on_working else orig, est, gen, lst, info=ti)
    status, verdict, polyA, polyadenil, recovered, kept, added, after, steps = t
    if status != OK:
        return settle(HOST, 4, 1)
    out.update(tail_added=added, polyA=polyA, polyadenil=polyadenil, recovered=recovered)
    if verdict != 0:
        return settle(EMPTY, 4, 1)
    lst = list(after) if keep_removed else TL.kept_exons(t)
    out["n_removed"] = len(after) - kept
    # ---- small (:1291-1305)
    if not lst or SL.einval(len(est), len(gen), lst, _one_query(est, len(lst))):
        return settle(HOST, 5, 2)
    s = info["small_answer"] = SL.small(orig, est, gen, lst, mil, ops=ops, info=si, clean_on_working=clean_on_working)
    status, refused, verdict, prefix_added, n_added, n_list, first, n_kept, after, steps = s
    if status != OK:
        out["refused"] = refused
        return settle(HOST, 5, 1)
    out.update(n_added=n_added, n_cleaned=n_list - n_kept, prefix_added=prefix_added)
    if verdict != 0:
        return settle(EMPTY, 5, verdict)
    out["exons"], out["steps"] = after[first:first + n_kept], steps[first:first + n_kept]
    return settle(DONE, 5, dropped)


def expect_arrays(answers):
    """answers of final() per EST -> (results, exons, steps) as the entry writes them"""
    from pintron_amd import capi
    res = np.zeros(len(answers), dtype=np.dtype(capi.FINAL_RESULT_DTYPE))
    ex, st = [], []
    for i, a in enumerate(answers):
        done = a["outcome"] == DONE
        for f in FIELDS:
            res[f][i] = a[f]
        res["first_exon"][i] = len(ex) if done else 0
        res["n_exons"][i] = len(a["exons"]) if done else 0
        if done:
            ex += [tuple(e) for e in a["exons"]]
            st += list(a["steps"])
    return res, np.array(ex, dtype=np.dtype(capi.FACTOR_DTYPE)).reshape(-1), np.array(st, dtype=np.uint8)


def batch_arrays(cases):
    """cases of (orig, est, exons) -- exons None or empty: no candidate -> (ests, exons array, queries array); equal strings
    are stored once"""
    from pintron_amd import capi
    n_ex = sum(len(c[2] or ()) for c in cases)
    exons = np.zeros(n_ex, dtype=np.dtype(capi.FACTOR_DTYPE))
    q = np.zeros(len(cases), dtype=np.dtype(capi.FINAL_QUERY_DTYPE))
    ests, eat, size, k = [], {}, 0, 0
    for i, (orig, est, ex) in enumerate(cases):
        ex = ex or ()
        for s in (est, orig):
            if s not in eat:
                eat[s] = size
                ests.append(s)
                size += len(s)
        for e in ex:
            exons[k] = tuple(e)
            k += 1
        q[i] = (eat[est], len(est), k - len(ex) if ex else 0, len(ex), 0, eat[orig])
    return b"".join(ests), exons, q


def plan_queries(pat_off, cand_res, orig_off=None):
    """the queries of the index form that name the candidates a plan fetched (as fact_lib.plan_queries); orig_off: one
    offset per pattern (None: the pattern's own)"""
    from pintron_amd import capi
    fq = F.plan_queries(pat_off, cand_res)
    q = np.zeros(len(fq), dtype=np.dtype(capi.FINAL_QUERY_DTYPE))
    for f in ("est_off", "est_len", "first_exon", "n_exons"):
        q[f] = fq[f]
    q["orig_off"] = fq["est_off"] if orig_off is None else orig_off
    return q


def stage0_of_kinds(res, kinds):
    """as fact_lib.stage0_of_kinds, for final results"""
    res = res.copy()
    for i in np.nonzero(kinds != KL.ONE)[0]:
        k = int(kinds[i])
        res[i] = np.zeros((), dtype=res.dtype)
        res["outcome"][i], res["detail"][i] = (EMPTY if k == KL.REFUSED else HOST), k
    return res


# ---- today's route: the three public entries one after the other, the glue on the host -------------------------------
def _tuples(arr):
    return [tuple(int(v) for v in e) for e in arr]


def _stage_batch(ests, queries, live, lists, dtype):
    """the queries `live` over their lists {i: [exons]}, as a call of their own"""
    from pintron_amd import capi
    ex = np.array([e for i in live for e in lists[i]], dtype=np.dtype(capi.FACTOR_DTYPE)).reshape(-1)
    q = np.zeros(len(live), dtype=np.dtype(dtype))
    k = 0
    for j, i in enumerate(live):
        q[j] = (int(queries["est_off"][i]), int(queries["est_len"][i]), k, len(lists[i]), 0, int(queries["orig_off"][i]))
        k += len(lists[i])
    return ex, q


def glue(idx, gen_len, ests: bytes, queries, fact, mil, clock=None):
    """the answer `fact` of the factorization stage (its three arrays) -> the arrays of expect_arrays, through
    pgpu_index_tail_chains and pgpu_index_small_chains with the host doing what the final driver does on the device.
    `clock` (a dict) receives "library_s", the seconds inside the two entries, and "kernel_ms" of the two."""
    import time
    from pintron_amd import capi
    fres, fex, _ = fact
    n = len(queries)
    inside, ms = 0.0, [0.0, 0.0]
    out = []
    for i in range(n):
        a = dict.fromkeys(FIELDS, 0)
        a.update(outcome=int(fres["outcome"][i]), stage=int(fres["stage"][i]), detail=int(fres["detail"][i]),
                 n_merged=int(fres["n_merged"][i]), total_edit=int(fres["total_edit"][i]), exons=[], steps=[])
        out.append(a)
    one = lambda i, k: [dict(est_off=0, est_len=int(queries["est_len"][i]), first_exon=0, n_exons=k, reserved=0, orig_off=0)]
    lists, live = {}, []
    for i in range(n):
        if out[i]["outcome"] != DONE:
            continue
        lo, k = int(fres["first_exon"][i]), int(fres["n_exons"][i])
        lst = _tuples(fex[lo:lo + k])
        out[i]["dropped"] = out[i]["detail"] & 1
        if TL.einval(int(queries["est_len"][i]), gen_len, lst, one(i, k)):
            out[i].update(outcome=HOST, stage=4, detail=2)
        else:
            lists[i] = lst
            live.append(i)
    if live:
        ex, q = _stage_batch(ests, queries, live, lists, capi.TAIL_QUERY_DTYPE)
        t0 = time.perf_counter()
        ex2, steps, res = idx.tail_chains(ests, ex, q)
        inside += time.perf_counter() - t0
        ms[0] = idx.tail_chains_kernel_ms()
        nxt = []
        for j, i in enumerate(live):
            a = out[i]
            if res["status"][j] != OK:
                a.update(outcome=HOST, stage=4, detail=1)
                continue
            a.update(tail_added=int(res["tail_added"][j]), polyA=int(res["polyA"][j]), polyadenil=int(res["polyadenil"][j]),
                     recovered=int(res["recovered"][j]))
            if res["verdict"][j] != 0:
                a.update(outcome=EMPTY, stage=4, detail=1)
                continue
            lo, k = int(q["first_exon"][j]), int(q["n_exons"][j])
            lst = [e for e, s in zip(_tuples(ex2[lo:lo + k]), steps[lo:lo + k]) if s & 3 != TL.REMOVED]
            a["n_removed"] = k - len(lst)
            if not lst or SL.einval(int(queries["est_len"][i]), gen_len, lst, one(i, len(lst))):
                a.update(outcome=HOST, stage=5, detail=2)
            else:
                lists[i] = lst
                nxt.append(i)
        live = nxt
    if live:
        ex, q = _stage_batch(ests, queries, live, lists, capi.SMALL_QUERY_DTYPE)
        t0 = time.perf_counter()
        ex2, steps, res = idx.small_chains(ests, ex, q, mil)
        inside += time.perf_counter() - t0
        ms[1] = idx.small_chains_kernel_ms()
        for j, i in enumerate(live):
            a = out[i]
            if res["status"][j] != OK:
                a.update(outcome=HOST, stage=5, detail=1, refused=int(res["refused"][j]))
                continue
            a.update(n_added=int(res["n_added"][j]), n_cleaned=int(res["n_list"][j]) - int(res["n_kept"][j]),
                     prefix_added=int(res["prefix_added"][j]))
            if res["verdict"][j] != 0:
                a.update(outcome=EMPTY, stage=5, detail=int(res["verdict"][j]))
                continue
            lo = 2 * int(q["first_exon"][j]) + int(res["first_kept"][j])
            k = int(res["n_kept"][j])
            a.update(outcome=DONE, stage=5, detail=a["dropped"], exons=_tuples(ex2[lo:lo + k]), steps=[int(s) for s in steps[lo:lo + k]])
    if clock is not None:
        clock["library_s"], clock["kernel_ms"] = inside, ms
    return expect_arrays(out)


def route(idx, gen_len, ests: bytes, exons, queries, prm=F.DEFAULTS, mil=None):
    """The arrays of expect_arrays from pgpu_index_factorizations, pgpu_index_tail_chains and pgpu_index_small_chains
    called one after the other."""
    from pintron_amd import capi
    fq = np.zeros(len(queries), dtype=np.dtype(capi.FACT_QUERY_DTYPE))
    for f in ("est_off", "est_len", "first_exon", "n_exons", "reserved"):
        fq[f] = queries[f]
    fact = idx.factorizations(ests, exons, fq, *prm)
    return glue(idx, gen_len, ests, queries, fact, int(prm[4]) if mil is None else mil)


# ---- what a case reached --------------------------------------------------------------------------------------------
def tags_of(answer, info, decided_by_orig=False):
    """the TAGS an answer of final() and its info show; decided_by_orig: the answer differs with the two sequences swapped
    for one (orig_decides costs a second computation: the caller makes it)"""
    ti, si = info.get("tail", {}), info.get("small", {})
    a = answer
    tags = set()
    reached_tail = "tail_answer" in info
    reached_small = "small_answer" in info
    if a["outcome"] == DONE and not (a["tail_added"] or a["recovered"] or a["n_removed"] or a["n_added"] or a["n_cleaned"]):
        tags.add("done_plain")
    if reached_tail:
        for t in ("affix_256", "affix_257", "window_128", "window_129", "gen_256", "gen_257", "exons_64", "exons_65"):
            if ti.get(t):
                tags.add("tail_" + t)
        t = info["tail_answer"]
        if t[0] == OK:
            if any(s & 3 == TL.REMOVED for s in t[8][2:]):
                tags.add("removed_reanalysed")
            if t[2]:
                tags.add("polyA")
            if t[3]:
                tags.add("polyadenil")
            if t[4] & 1:
                tags.add("recovered_prefix")
            if t[4] & 2:
                tags.add("recovered_suffix")
            if t[6]:
                tags.add("tail_added")
    if (a["outcome"], a["stage"]) == (EMPTY, 4):
        tags.add("empty_4")
    if (a["outcome"], a["stage"], a["detail"]) == (HOST, 4, 2):
        tags.add("host_4_validator")
    if reached_small:
        s = info["small_answer"]
        if s[0] != OK:
            tags.add("small_refused_%d" % s[1])
        for t in ("window_256", "window_257", "kband_31", "kband_32", "grow_past_64"):
            if si.get(t):
                tags.add(t if t == "grow_past_64" else "small_" + t)
        if s[0] == OK and s[3]:
            tags.add("prefix_exon")
        if s[0] == OK and s[4] - s[3] > 0:
            tags.add("between_exon")
    if (a["outcome"], a["stage"]) == (EMPTY, 5):
        tags.add("empty_5_noisy" if a["detail"] == 1 else "empty_5_external")
    if decided_by_orig:
        tags.add("orig_decides")
    return tags


# ---- the cases the GPU tests use ------------------------------------------------------------------------------------
PER_TAG = 4           # cases kept of each tag: one more than the cover asks for
_groups = []


def _answer(c, g, ops, **how):
    info = {}
    return final(KL.ONE if c["exons"] else KL.NONE, c["orig"], c["est"], g, c["exons"], c["prm"], c["mil"], ops=ops, info=info, **how), info


def own_world(seed=20261, reps=2 * MIN_PER_TAG):
    """(sequence, [case dicts]): what the two fixtures' cases do not bring through the stages 0-3, built with their builders
    over loci of small_lib.World -- exons that are exact copies, so that clean, gaps and refine leave them as they are, and
    the situation the later stages meet made by the ORIGINAL sequence or by bytes outside the exons:
      kband_1033 / kband_1034   a last exon of 1 000 bytes that step 1 of tail extends by 33 / 34: the K-band bound of small's
                                step 3 is 31 / 32, a cap clean met at 1 000 bytes with room to spare;
      grow_64                   64 exons, the first one with a small exon lost in front of it: tail sees its cap's last accepted
                                value, small's list grows to 65;
      window_256 / window_257   small_lib's prefix windows with enough exons behind them for clean's coverage rule;
      external                  two end exons of 15 bytes with both splice sites, the original differing in each by a byte:
                                clean keeps them on the working sequence, small's step 3 drops both on the original;
      affix_256                 a lost prefix window of 256 bytes in front of exons long enough for the coverage rule;
      suffix                    behind the last exon the original matches the sequence for k bytes and differs at the next,
                                the working sequence differs at the k-th and matches behind it: step 1 of tail extends the
                                exon over the original's k bytes, onto a byte where the working sequence differs, and step 4
                                recovers the suffix behind it (on equal sequences step 1 always stops on a matching byte)."""
    w = SL.World(seed, 44 * reps + 4)
    rng, g = w.rng, w.g
    cases = []

    def add(name, est, exons, orig=None, mil=None):
        est = bytes(est)
        cases.append(dict(name=name, orig=est if orig is None else bytes(orig), est=est, exons=[tuple(int(v) for v in e) for e in exons],
                          prm=F.DEFAULTS, mil=mil))

    def run_of_exons(at, n, size=40, intron=120):
        """n exons of `size` bytes copied from g[at ..), `intron` bytes apart -> (their bytes, [(offset in them, genomic start)])"""
        est, where = bytearray(), []
        for _ in range(n):
            where.append((len(est), at))
            est += g[at:at + size]
            at += size + intron
        return bytes(est), where

    for rep in range(reps):
        for extra in (33, 34):
            L = w.locus()
            w.locus()
            est = bytes(g[L.s:L.s + 1000 + extra]) + bytes([SL.other_base(g[L.s + 1000 + extra])]) + b"CT"
            add("kband_%d" % (1000 + extra), est, [(0, 999, L.s, L.s + 999)])
        # [S] GT .. AG [A] and 63 exons behind: the factorization begins at A
        L = w.locus(s_len=12)
        room = [w.locus() for _ in range(8)]
        est, ex = SL.prefix_case(L)
        more, where = run_of_exons(room[0].s, 63)
        exons = list(ex) + [(len(est) + o, len(est) + o + 39, at, at + 39) for o, at in where]
        add("grow_64", est + more + b"TTGACCA", exons, mil=40)
        for allelen in (256, 257):
            L = w.locus(s_len=12, a_len=80, b_len=80, z_len=60)
            flank = SL.RL.rnd(rng, allelen - 23 - 46) + L.seq(L.s, 12) + SL.RL.rnd(rng, 22)
            est, ex = SL.prefix_case(L, flank=flank)
            e0 = len(est)
            est += L.seq(L.b, 80) + L.seq(L.z, 60)
            add("window_%d" % allelen, est, list(ex) + [(e0, e0 + 79, L.b, L.b + 79), (e0 + 80, e0 + 139, L.z, L.z + 59)], mil=40)
        L = w.locus(s_len=15, a_len=15)
        est = L.seq(L.s, 15) + L.seq(L.a, 15)
        orig = bytearray(est)
        orig[7], orig[22] = SL.other_base(orig[7]), SL.other_base(orig[22])
        add("external", est, [(0, 14, L.s, L.s + 14), (15, 29, L.a, L.a + 14)], orig=orig)
        L = w.locus()
        room = w.locus()
        at = L.s + 300
        flank = bytearray(g[at - 256:at])
        flank[-1] = SL.other_base(flank[-1])
        body, ex, end = TL.chain(g, at, [120, (b"", 200), 150, (b"", 150), 130], flank=bytes(flank))
        add("affix_256", bytes(body) + bytes([SL.other_base(g[end])]) + b"GA", ex)
        L = w.locus()
        w.locus()
        k = (1, 5, 12)[rep % 3]
        body, ex, end = TL.chain(g, L.s + 200, [120, (b"", 200), 150])
        est = bytes(body) + bytes(g[end:end + k - 1]) + bytes([SL.other_base(g[end + k - 1])]) + bytes(g[end + k:end + k + 40]) + \
            bytes([SL.other_base(g[end + k + 40])]) + b"CT"
        orig = bytearray(est)
        orig[len(body) + k - 1], orig[len(body) + k] = g[end + k - 1], SL.other_base(g[end + k])
        add("suffix", est, ex, orig=orig)
    return bytes(g), cases


def candidate_pool():
    """[(sequence name, sequence, [case: name, orig, est, exons, prm, mil])]: every hand-made case of the tail fixture and of
    the small fixture's worlds, and the hand-made candidates of fact_lib, each over its own sequence"""
    pool = []
    g, cases, _ = TL.load_fixture()
    pool.append(("tail", g, [dict(name=c["name"], orig=c["orig"], est=c["est"], exons=c["exons"], prm=F.DEFAULTS, mil=None) for c in cases]))
    for k, (g, cases) in enumerate(SL.load_fixture()[0]):
        pool.append(("small%d" % k, g, [dict(name=c["name"], orig=c["orig"], est=c["est"], exons=c["exons"],
                                             prm=F.DEFAULTS[:4] + (c["mil"],), mil=c["mil"]) for c in cases]))
    g, cases = F.hand_cases()
    pool.append(("fact", g, [dict(name=n, orig=est, est=est, exons=ex, prm=prm, mil=None) for n, est, ex, prm, _ in cases]))
    pool.append(("own",) + own_world())
    return pool


def hand_groups():
    """[(sequence name, sequence, [case dicts with "answer", "info" and "tags"])]: of the pool, the first PER_TAG cases that
    reach each tag, in the pool's order.  Computed once.  Shared: do not modify."""
    if not _groups:
        for name, g, cases in candidate_pool():
            ops = SL.OracleOps(g)
            seen, kept = {}, []
            for c in cases:
                c["answer"], c["info"] = _answer(c, g, ops)
                swapped = False
                if c["orig"] != c["est"]:
                    swapped = _answer(dict(c, orig=c["est"]), g, ops)[0] != c["answer"]
                c["tags"] = tags_of(c["answer"], c["info"], swapped)
                a = c["answer"]                                  # ... and of every outcome that is not DONE, by its cell
                keys = set(c["tags"]) | ({(a["outcome"], a["stage"], a["detail"])} if a["outcome"] != DONE else set())
                if any(seen.get(t, 0) < PER_TAG for t in keys):
                    for t in keys:
                        seen[t] = seen.get(t, 0) + 1
                    kept.append(c)
            _groups.append((name, g, kept))
    return _groups


def by_settings(cases):
    """{(prm, mil): [cases]}: the cases of one call each"""
    out = {}
    for c in cases:
        out.setdefault((c["prm"], int(c["prm"][4]) if c["mil"] is None else c["mil"]), []).append(c)
    return out


# ---- the hand-off kernels over made-up stage results ----------------------------------------------------------------
# What NOT_REACHED names cannot arrive through clean, gaps and refine, so the branches of the three hand-off kernels that
# carry it are run over stage results made by hand (pgpu_final_handoffs_probe: no stage kernel runs, no EST byte is read)
# and compared with the same glue written here.  A case: est_len, fact = (outcome, stage, detail, n_merged, total_edit),
# exons (DONE only), tail = the fields of pgpu_tail_result, tail_exons / tail_steps (parallel to exons), small = the fields
# of pgpu_small_result, small_list / small_steps (at most twice as many), tags.
PROBE_GEN_LEN = 10_000


def _run(k, at=0):
    return [(at + 3 * i, at + 3 * i + 1, 10 * i, 10 * i + 1) for i in range(k)]


def probe_cases():
    out = []
    ok_tail = lambda k, **kw: dict(dict(status=0, verdict=0, polyA=0, polyadenil=0, recovered=0, n_kept=k, tail_added=0), **kw)
    ok_small = lambda k, **kw: dict(dict(status=0, refused=0, verdict=0, prefix_added=0, n_added=0, n_list=k, first_kept=0, n_kept=k), **kw)
    erange_tail = dict(status=-34, verdict=0, polyA=0, polyadenil=0, recovered=0, n_kept=0, tail_added=0)

    def add(tags, exons, tail=None, small=None, tail_exons=None, tail_steps=None, small_list=None, small_steps=None, est_len=400,
            fact=(DONE, 3, 0, 0, 0)):
        k = len(exons)
        tail_exons = list(exons) if tail_exons is None else tail_exons
        tail_steps = [0] * k if tail_steps is None else tail_steps
        kept = [e for e, s_ in zip(tail_exons, tail_steps) if s_ & 3 != TL.REMOVED]
        small_list = kept if small_list is None else small_list
        out.append(dict(tags=set(tags), est_len=est_len, fact=fact, exons=list(exons), tail=tail or ok_tail(len(kept)),
                        tail_exons=tail_exons, tail_steps=tail_steps, small=small or ok_small(len(small_list)),
                        small_list=small_list, small_steps=[0] * len(small_list) if small_steps is None else small_steps))

    for rep, k in enumerate((65, 66, 100)):
        add({"tail_exons_65"}, _run(k), tail=erange_tail)
        add({"tail_window_129"}, _run(3 + rep), tail=erange_tail)
        add({"tail_gen_257"}, _run(4 + rep), tail=erange_tail, fact=(DONE, 3, 1, rep, 7))
        add({"tail_window_128", "tail_gen_256"}, _run(3 + rep), tail=ok_tail(3 + rep, tail_added=rep))
    # a coordinate equal to a length: each of the four fields, and the last accepted value beside it
    e = _run(3)
    add({"host_4_validator"}, e[:2] + [(e[2][0], 400, e[2][2], e[2][3])])
    add({"host_4_validator"}, [(400, e[0][1], e[0][2], e[0][3])] + e[1:])
    add({"host_4_validator"}, e[:2] + [(e[2][0], e[2][1], e[2][2], PROBE_GEN_LEN)])
    add({"host_4_validator"}, e[:1] + [(e[1][0], e[1][1], PROBE_GEN_LEN, e[1][3])] + e[2:])
    add({"host_4_validator"}, e, est_len=0)
    add(set(), e[:2] + [(e[2][0], 399, e[2][2], PROBE_GEN_LEN - 1)])
    # verdict 1 of tail keeps the flags and tail_added; a recovered suffix, alone and with a prefix
    for polyA, polyadenil, added in ((1, 0, 0), (1, 1, 9), (0, 0, 300)):
        add({"empty_4"}, _run(2 + added % 4), tail=ok_tail(0, verdict=1, polyA=polyA, polyadenil=polyadenil, tail_added=added))
    for recovered, k in ((2, 1), (3, 2), (2, 5)):
        ex = _run(k)
        moved = ex[:-1] + [(ex[-1][0], ex[-1][1] + 4, ex[-1][2], ex[-1][3] + 4)]
        add({"recovered_suffix"}, ex, tail=ok_tail(k, recovered=recovered), tail_exons=moved, tail_steps=[0] * (k - 1) + [TL.STEP_SUFFIX])
    # every refusal of small, behind a tail stage that removed an exon
    for code in (1, 2, 3, 4, 5):
        for k in (3, 4, 64):
            steps = [0, TL.REMOVED] + [0] * (k - 2)
            add({"small_refused_%d" % code}, _run(k), tail=ok_tail(k - 1, recovered=1, polyA=1), tail_steps=steps,
                small=dict(status=-34, refused=code, verdict=0, prefix_added=0, n_added=0, n_list=0, first_kept=0, n_kept=0))
    # what tail hands over is tested again: a coordinate it moved out of its string, and a list it emptied
    ex = _run(3)
    add(set(), ex, tail_exons=[ex[0], ex[1], (ex[2][0], 400, ex[2][2], ex[2][3])])
    add(set(), ex, tail=ok_tail(0), tail_steps=[TL.REMOVED] * 3)
    # small's verdicts, a kept run in the middle of a list that grew, and the outcomes of the stages 0-3 carried over
    ex = _run(4)
    grown = [ex[0], (20, 21, 30, 31), ex[1], ex[2], (50, 51, 60, 61), ex[3]]
    for verdict in (1, 2):
        add(set(), ex, small=ok_small(6, verdict=verdict, n_added=2, prefix_added=1, first_kept=0, n_kept=0), small_list=grown)
    add(set(), ex, small=ok_small(6, n_added=2, first_kept=1, n_kept=4), small_list=grown, small_steps=[0, 2, 4, 4, 2, 32],
        fact=(DONE, 3, 1, 2, 5))
    add(set(), ex, tail_steps=[0, TL.REMOVED, TL.REMOVED, 0], small=ok_small(4, n_added=2, first_kept=0, n_kept=4), small_list=grown[:4])
    for fact in ((HOST, 0, 1, 0, 0), (EMPTY, 0, 2, 0, 0), (EMPTY, 1, 7, 0, 0), (HOST, 2, 1, 0, 0), (EMPTY, 2, 1, 0, 33), (HOST, 3, 1, 0, 12)):
        add(set(), [], fact=fact)
    return out


def probe_arrays(cases):
    """cases of probe_cases() -> the arguments of capi.final_handoffs_probe"""
    from pintron_amd import capi
    n = len(cases)
    E = sum(len(c["exons"]) for c in cases) + 3                     # (three exons at the end that no EST names)
    q = np.zeros(n, dtype=np.dtype(capi.FINAL_QUERY_DTYPE))
    fres = np.zeros(n, dtype=np.dtype(capi.FACT_RESULT_DTYPE))
    fex = np.zeros(E, dtype=np.dtype(capi.FACTOR_DTYPE))
    tres = np.zeros(n, dtype=np.dtype(capi.TAIL_RESULT_DTYPE))
    tex, tst = np.zeros(E + n, dtype=fex.dtype), np.zeros(E + n, dtype=np.uint8)
    sres = np.zeros(n, dtype=np.dtype(capi.SMALL_RESULT_DTYPE))
    sex, sst = np.zeros(2 * (E + n), dtype=fex.dtype), np.zeros(2 * (E + n), dtype=np.uint8)
    at = off = 0
    for i, c in enumerate(cases):
        k = len(c["exons"])
        q[i] = (off, c["est_len"], 0, 0, 0, off)
        off += c["est_len"]
        o, s_, d, merged, edit = c["fact"]
        fres[i] = (o, s_, d, at if k else 0, k, merged, edit)
        for f in tres.dtype.names:
            tres[f][i] = c["tail"][f]
        for f in sres.dtype.names:
            sres[f][i] = c["small"].get(f, 0)
        for j in range(k):
            fex[at + j], tex[at + j], tst[at + j] = c["exons"][j], c["tail_exons"][j], c["tail_steps"][j]
        for j, e in enumerate(c["small_list"]):
            sex[2 * at + j], sst[2 * at + j] = e, c["small_steps"][j]
        at += k
    return dict(q=q, ests_len=off, fres=fres, fex=fex, tres=tres, tex=tex, tst=tst, sres=sres, sex=sex, sst=sst)


def probe_expect(cases):
    """the glue of final() over the made-up results -> (the arrays of expect_arrays, the exon count of each small query)"""
    out, asked = [], []
    for c in cases:
        a = dict.fromkeys(FIELDS, 0)
        o, s_, d, merged, edit = c["fact"]
        a.update(outcome=o, stage=s_, detail=d, n_merged=merged, total_edit=edit, exons=[], steps=[])
        out.append(a)
        asked.append(1)
        if o != DONE:
            continue
        one = lambda k: [dict(est_off=0, est_len=c["est_len"], first_exon=0, n_exons=k, reserved=0, orig_off=0)]
        if TL.einval(c["est_len"], PROBE_GEN_LEN, c["exons"], one(len(c["exons"]))):
            a.update(outcome=HOST, stage=4, detail=2)
            continue
        t = c["tail"]
        if t["status"] != OK:
            a.update(outcome=HOST, stage=4, detail=1)
            continue
        a.update(tail_added=t["tail_added"], polyA=t["polyA"], polyadenil=t["polyadenil"], recovered=t["recovered"])
        if t["verdict"]:
            a.update(outcome=EMPTY, stage=4, detail=1)
            continue
        kept = [e for e, st in zip(c["tail_exons"], c["tail_steps"]) if st & 3 != TL.REMOVED]
        a["n_removed"] = len(c["exons"]) - len(kept)
        if not kept or SL.einval(c["est_len"], PROBE_GEN_LEN, kept, one(len(kept))):
            a.update(outcome=HOST, stage=5, detail=2)
            continue
        asked[-1] = len(kept)
        s = c["small"]
        if s["status"] != OK:
            a.update(outcome=HOST, stage=5, detail=1, refused=s["refused"])
            continue
        a.update(n_added=s["n_added"], n_cleaned=s["n_list"] - s["n_kept"], prefix_added=s["prefix_added"])
        if s["verdict"]:
            a.update(outcome=EMPTY, stage=5, detail=s["verdict"])
            continue
        lo, k = s["first_kept"], s["n_kept"]
        a.update(outcome=DONE, stage=5, detail=d & 1, exons=c["small_list"][lo:lo + k], steps=c["small_steps"][lo:lo + k])
    return expect_arrays(out), asked
