"""CPU restatement of the list stage (pgpu_index_factorization_lists, pgpu_pairing_plan_run_factorization_lists,
pintron_amd/csrc/pgpu_flists.hip): the candidates of one EST through clean_lib, add_if_not_exists with
relaxed_list_contained and relaxed_factor_compare (src/list.c:320-483, src/est-factorizations.c:1159-1259, :2041-2109),
FILTER 1 and FILTER 3, gaps_lib per entry with max_number_of_factorizations, and chain_lib per entry, with the glue of
fact_lib.  Shared by tests/test_flists_cpu.py, tests/test_gpu_flists.py, tools/make_flists_golden.py and
tools/flists_cost.py.

factorization_list  one EST and its candidates -> answer(); `wrong` names a rule a wrong implementation might have instead.
tags_of             what a case exercised, from the `info` the restatement filled.
expect_arrays       answers -> the four arrays of the entry.
batch_arrays        cases -> (ests, candidate table, exons, queries).
hand_cases          hand-made cases over hand_sequence(), a seeded 30 kb sequence with the repeats some cases need planted.
Host                the host's ef_chain_factorizations through tests/hostcheck/libestfact_check.so.
"""
import gzip
import json
import os

import numpy as np

import chain_lib as RC
import clean_lib as CL
import fact_lib as FL
import gaps_lib as GL

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "factorization_lists.json.gz")

HOST, EMPTY, DONE = 0, 1, 2
OK = 0
MERGED = 0x80
MAX_CANDIDATES, CAP_CANDIDATES = 64, 4
DROPPED_FIRST, HEAD_WIDENED, TAIL_WIDENED = 1, 2, 4
# complexity_threshold, suffpref on_est / for_intron / on_gen, min_intron_length, max_coverage_diff, max_site_difference,
# max_gaplength_diff, max_number_of_factorizations: the reference's defaults
DEFAULTS = FL.DEFAULTS + (0.05, 50, 20, 0)

WRONG_RULES = ("no_widening", "remove_behind_stop", "filter3_first", "filters_on_uncleaned", "max_number_first", "cfr_type_0")

TAGS = ("one_-2", "one_-1", "one_1", "one_0", "list_-2", "list_-1", "list_1", "list_0",
        "cfr_0", "cfr_-2", "cfr_-1", "cfr_2_match", "cfr_2_unconf", "cfr_2_tot", "cfr_2_walked", "cfr_1_match", "cfr_1_unconf",
        "cfr_1_tot", "cfr_1_walked", "widen_head", "widen_tail", "widen_both", "removal_then_append", "removal_then_stop",
        "f1_diff", "f1_abs", "f1_noop", "f3_removed", "f3_noop", "f3_off", "max_number_at", "max_number_above",
        "gaps_drop_one", "gaps_drop_all", "filtered_before_cap", "cands_64", "cands_65", "no_candidate",
        "host_1_1", "host_1_2", "host_3_1", "host_3_2", "host_4_1", "empty_1", "done_2_or_more", "dropped_one_of_two")
# HOST at stage 4 with detail 2 (two kept exons out of order) has no tag: gaps_kernel cannot write such a list -- its border
# loop sets a.EST_start = d.EST_end + 1 behind every EST gap and leaves an empty gap's ends, which the query's validator has
# seen in order; its merging loop keeps an exon only when it begins more than 3 bases behind its donor's GEN_end and gives a
# merged exon's ends to the donor -- so the branch is run over gaps results made by hand (with_given_gaps,
# pgpu_flist_handoffs_probe; tests/test_gpu_flists.py)


def params(**kw):
    names = ("complexity_threshold", "suffpref_length_on_est", "suffpref_length_for_intron", "suffpref_length_on_gen",
             "min_intron_length", "max_coverage_diff", "max_site_difference", "max_gaplength_diff", "max_number_of_factorizations")
    p = list(DEFAULTS)
    for k, v in kw.items():
        p[names.index(k)] = v
    return tuple(p)


def capi_params(prm):
    from pintron_amd import capi
    return capi.flist_params(*prm)


# ---- add_if_not_exists -----------------------------------------------------------------------------------------------
def relaxed_factor_compare(p1, p2, cfr_type, allowed, l1, info):
    """src/est-factorizations.c:1159-1259; exons are (EST_start, EST_end, GEN_start, GEN_end); p1 is an exon of l1"""
    if p1[2] < p2[2] and p1[3] < p2[2]:
        return 1
    if p2[2] < p1[2] and p2[3] < p1[2]:
        return 1
    max_unconf = 20
    if cfr_type == 0:
        info["cfr_0"] = True
        if abs(p1[3] - p2[3]) <= allowed and abs(p1[2] - p2[2]) <= allowed:
            return 0
    if abs(cfr_type) == 2:
        if abs(p1[3] - p2[3]) <= allowed:
            if cfr_type == 2:
                d = p1[2] - p2[2]
                if d > max_unconf:
                    info["cfr_2_unconf"] = True
                    return 1
                if d > 0:
                    tot = 0
                    for f in l1:
                        if p1[2] == f[2]:
                            break
                        tot += f[3] - f[2] + 1
                    if abs(d - tot) < 10:
                        info["cfr_2_tot"] = True
                        return 1
                    info["cfr_2_walked"] = True
                info["cfr_2_match"] = True
            else:
                info["cfr_-2"] = True
            return 0
    if abs(cfr_type) == 1:
        if abs(p1[2] - p2[2]) <= allowed:
            if cfr_type == 1:
                d = p2[3] - p1[3]
                if d > max_unconf:
                    info["cfr_1_unconf"] = True
                    return 1
                if d > 0:
                    tot = 0
                    for f in reversed(l1):
                        if p1[2] == f[2]:
                            break
                        tot += f[3] - f[2] + 1
                    if abs(d - tot) < 20:
                        info["cfr_1_tot"] = True
                        return 1
                    info["cfr_1_walked"] = True
                info["cfr_1_match"] = True
            else:
                info["cfr_-1"] = True
            return 0
    return 1


def relaxed_list_contained(a, b, allowed, info, flat=False):
    """src/list.c:320-483 with a = to_add, b = the entry: 0 different, -1 a in b, 1 b in a, -2 equal.  flat: the wrong rule
    `cfr_type 0 everywhere`."""
    t = (lambda x: 0) if flat else (lambda x: x)
    if len(a) == len(b):
        if len(a) == 1:
            return 0
        for k in range(len(a)):
            typ = -2 if k == 0 else (-1 if k == len(a) - 1 else 0)
            if relaxed_factor_compare(a[k], b[k], t(typ), allowed, a, info) != 0:
                return 0
        return -2
    if len(a) == 1 or len(b) == 1:
        return 0
    a_longer = len(a) > len(b)
    lng, sht = (a, b) if a_longer else (b, a)
    il = i_s = 0
    typ, count_long, found = -2, 1, False
    while il < len(lng) and not found:
        if relaxed_factor_compare(lng[il], sht[i_s], t(typ), allowed, lng, info) == 0:
            found = True
            i_s += 1
        else:
            count_long += 1
        il += 1
        if typ == -2:
            typ = 2
    if not found:
        return 0
    count_factors, stop = 1, False
    while il < len(lng) and i_s < len(sht) and not stop:
        typ = (-1 if count_long + 1 == len(lng) else 1) if count_factors + 1 == len(sht) else 0
        if relaxed_factor_compare(lng[il], sht[i_s], t(typ), allowed, lng, info) == 0:
            il += 1
            i_s += 1
        else:
            stop = True
        count_factors += 1
        count_long += 1
    if stop:
        return 0
    if count_factors != len(sht):
        return 0
    return 1 if a_longer else -1


def res_of(a, b, allowed, info, flat=False):
    if len(a) == 1 and len(b) == 1:
        h1, h2 = a[0], b[0]
        if h1[2] == h2[2] and h1[3] == h2[3]:
            r = -2
        elif h1[2] >= h2[2] and h1[3] <= h2[3]:
            r = -1
        elif h1[2] <= h2[2] and h1[3] >= h2[3]:
            r = 1
        else:
            r = 0
        info["one_%d" % r] = True
        return r
    r = relaxed_list_contained(a, b, allowed, info, flat)
    info["list_%d" % r] = True
    return r


def add_if_not_exists(flist, entry, allowed, info, wrong=None):
    """:2041-2109 on flist, a list of dict(idx, exons (lists, changed in place by the widening), flags)"""
    to_add = entry["exons"]
    found, removed, k = False, False, 0
    while k < len(flist) and not found:
        cmp = flist[k]
        r = res_of(to_add, cmp["exons"], allowed, info, flat=wrong == "cfr_type_0")
        if r < 0:
            if r == -2 and wrong != "no_widening":
                h1, h2, t1, t2 = to_add[0], cmp["exons"][0], to_add[-1], cmp["exons"][-1]
                head = h1[0] < h2[0]
                if head:
                    h2[0], h2[2] = h1[0], h1[2]
                    cmp["flags"] |= HEAD_WIDENED
                tail = t1[1] > t2[1]
                if tail:
                    t2[1], t2[3] = t1[1], t1[3]
                    cmp["flags"] |= TAIL_WIDENED
                if head or tail:
                    info["widened"] = info.get("widened", 0) + 1
                    info["widen_both" if head and tail else ("widen_head" if head else "widen_tail")] = True
            found = True
            if removed:
                info["removal_then_stop"] = True
        elif r == 1:
            del flist[k]
            removed = True
            continue
        k += 1
    if found and wrong == "remove_behind_stop":
        flist[k:] = [c for c in flist[k:] if res_of(to_add, c["exons"], allowed, {}, False) != 1]
    if not found:
        flist.append(entry)
        if removed:
            info["removal_then_append"] = True


def coverage(exons, est_len):
    cover = est_len - (exons[0][0] + (est_len - exons[-1][1] - 1))       # :1262-1273, in int
    return float(cover) / float(est_len)


def filter1(flist, est_len, max_coverage_diff, info, key="exons"):
    cov, max_cov = [], 0.0
    for e in flist:
        x = e[key]
        if len(x) == 1 and (x[0][0] < 0 or x[0][0] >= est_len):
            cov.append(-1.0)
            continue
        cov.append(coverage(x, est_len))
        if max_cov < cov[-1]:
            max_cov = cov[-1]
    out = []
    for e, c in zip(flist, cov):
        if c == -1.0 or max_cov - c > max_coverage_diff:
            info["f1_diff"] = True
        elif (max_cov - c) * est_len > 100:
            info["f1_abs"] = True
        else:
            out.append(e)
    if len(out) == len(flist) and len(flist) > 1:
        info["f1_noop"] = True
    return out


def gap_length(exons):
    return sum(a[0] - d[1] - 1 for d, a in zip(exons, exons[1:]))


def filter3(flist, max_gaplength_diff, info, key="exons"):
    gl = [gap_length(e[key]) for e in flist]
    min_gl = -1
    for g in gl:
        if min_gl == -1 or min_gl > g:                           # as :389-392: a minimum of -1 is taken for "none yet"
            min_gl = g
    out = [e for e, g in zip(flist, gl) if not (max_gaplength_diff != -1 and g - min_gl > max_gaplength_diff)]
    if len(flist) > 1:
        info["f3_off" if max_gaplength_diff == -1 else ("f3_removed" if len(out) < len(flist) else "f3_noop")] = True
    return out


# ---- the stage ---------------------------------------------------------------------------------------------------------
def answer(outcome, stage, detail, counts=(0, 0, 0), facts=()):
    return dict(outcome=outcome, stage=stage, detail=detail, counts=tuple(counts), facts=list(facts))


def _query(est, n):
    return [dict(est_off=0, est_len=len(est), first_exon=0, n_exons=n, reserved=0)]


def factorization_list(est: bytes, gen: bytes, cands, prm=DEFAULTS, info=None, wrong=None, given_gaps=None):
    """One EST and its candidates [[(EST_start, EST_end, GEN_start, GEN_end)]] in the enumeration stage's order -> answer():
    outcome, stage, detail, counts = (n_cleaned, n_listed, n_filtered), facts = [dict(candidate (index into cands), exons,
    steps, n_merged, total_edit, flags)].  given_gaps {candidate index: (status, verdict, total_edit, exons afterwards,
    steps)} stands in for gaps_lib.gaps on those candidates."""
    info = {} if info is None else info
    thr, settings = prm[0], tuple(prm[1:5])
    max_cov_diff, allowed, max_gl_diff, max_n = prm[5], int(prm[6]), prm[7], prm[8]
    m = len(cands)
    info["m"] = m
    if m == 0:
        return answer(EMPTY, 0, 0)
    if m > MAX_CANDIDATES:
        return answer(HOST, 0, CAP_CANDIDATES)
    # ---- 1. clean, per candidate; the lowest index decides
    survivors = []
    for idx, ex in enumerate(cands):
        lst = [tuple(int(v) for v in e) for e in ex]
        if CL.einval(len(est), len(gen), lst, _query(est, len(lst))):
            return answer(HOST, 1, 2)
        status, verdict, first, n, after, marks = CL.clean(est, gen, lst, thr)
        if status != OK:
            return answer(HOST, 1, 1)
        if verdict == 0:
            survivors.append(dict(idx=idx, exons=[list(e) for e in after[first:first + n]], flags=0, raw=lst))
    n_cleaned = len(survivors)
    if not survivors:
        return answer(EMPTY, 1, 0, (0, 0, 0))
    # ---- 2. select
    info["cleaned"] = [[tuple(x) for x in e["exons"]] for e in survivors]
    flist = []
    for e in survivors:
        add_if_not_exists(flist, e, allowed, info, wrong)
    info["selected"] = [[tuple(x) for x in e["exons"]] for e in flist]
    n_listed = len(flist)
    info["listed"] = n_listed
    key = "raw" if wrong == "filters_on_uncleaned" else "exons"
    if wrong == "filter3_first":
        flist = filter1(filter3(flist, max_gl_diff, info, key), len(est), max_cov_diff, info, key)
    else:
        flist = filter3(filter1(flist, len(est), max_cov_diff, info, key), max_gl_diff, info, key)
    n_filtered = len(flist)
    counts = (n_cleaned, n_listed, n_filtered)
    for e in survivors:                                              # (for the tags: what a filter kept from a later cap)
        lst = [tuple(x) for x in e["exons"]]
        if wrong is None and not any(e is k for k in flist) and not GL.einval(len(est), len(gen), lst, _query(est, len(lst))) \
                and GL.gaps(est, gen, lst)[0] != OK:
            info["filtered_before_cap"] = True
    if wrong == "max_number_first" and max_n != 0 and len(flist) > max_n:
        return answer(EMPTY, 3, 2, counts)
    # ---- 3. gaps, FILTER 4; the lowest index decides
    left = []
    for e in flist:
        lst = [tuple(x) for x in e["exons"]]
        if GL.einval(len(est), len(gen), lst, _query(est, len(lst))):
            return answer(HOST, 3, 2, counts)
        if given_gaps is not None and e["idx"] in given_gaps:      # (what pgpu_flist_handoffs_probe does on the device)
            status, verdict, total, after, steps = given_gaps[e["idx"]]
        else:
            status, verdict, total, kept, after, steps = GL.gaps(est, gen, lst)
        if status != OK:
            return answer(HOST, 3, 1, counts)
        if verdict != 0:
            info["gaps_dropped"] = info.get("gaps_dropped", 0) + 1
            continue
        kept_ex = [x for x, s in zip(after, steps) if not s & MERGED]
        left.append(dict(e, exons=kept_ex, n_merged=len(after) - len(kept_ex), total_edit=total))
    info["left"] = len(left)
    if not left:
        return answer(EMPTY, 3, 1, counts)
    if max_n != 0:
        info["max_number_at" if len(left) == max_n else ("max_number_above" if len(left) > max_n else "max_number_below")] = True
        if len(left) > max_n:
            return answer(EMPTY, 3, 2, counts)
    # ---- 4. refine
    facts = []
    for e in left:
        lst = e["exons"]
        if any(d[1] >= a[0] or d[3] >= a[2] for d, a in zip(lst, lst[1:])):
            return answer(HOST, 4, 2, counts)
        status, done, dropped, after, steps = RC.chain(est, gen, lst, settings)
        if status != OK:
            return answer(HOST, 4, 1, counts)
        if dropped:
            after, steps = after[1:], steps[1:]
        facts.append(dict(candidate=e["idx"], exons=[tuple(x) for x in after], steps=[int(s) for s in steps], n_merged=e["n_merged"],
                          total_edit=e["total_edit"], flags=e["flags"] | (DROPPED_FIRST if dropped else 0)))
    return answer(DONE, 4, 0, counts, facts)


def tags_of(ans, info):
    t = {k for k in TAGS if info.get(k)}
    if ans["outcome"] == HOST and ans["stage"] in (1, 3, 4):
        t.add("host_%d_%d" % (ans["stage"], ans["detail"]))
    if ans["outcome"] == EMPTY and ans["stage"] == 1:
        t.add("empty_1")
    if ans["outcome"] == EMPTY and ans["stage"] == 0:
        t.add("no_candidate")
    if ans["outcome"] == DONE and len(ans["facts"]) >= 2:
        t.add("done_2_or_more")
        if len({f["flags"] & DROPPED_FIRST for f in ans["facts"]}) == 2:
            t.add("dropped_one_of_two")
    if info.get("gaps_dropped"):
        t.add("gaps_drop_all" if info.get("left") == 0 else "gaps_drop_one")
    if info.get("m") == 64:
        t.add("cands_64")
    if info.get("m") == 65:
        t.add("cands_65")
    return sorted(t & set(TAGS))


# ---- arrays ------------------------------------------------------------------------------------------------------------
def batch_arrays(cases):
    """cases of (est, cands) -> (ests, candidate table, exons, queries); equal ESTs are stored once"""
    from pintron_amd import capi
    n_c = sum(len(c[1]) for c in cases)
    n_e = sum(len(x) for c in cases for x in c[1])
    cands = np.zeros(n_c, dtype=np.dtype(capi.ENUM_CANDIDATE_DTYPE))
    exons = np.zeros(n_e, dtype=np.dtype(capi.FACTOR_DTYPE))
    q = np.zeros(len(cases), dtype=np.dtype(capi.FLIST_QUERY_DTYPE))
    ests, eat, eoff, kc, ke = [], {}, 0, 0, 0
    for i, (est, cl) in enumerate(cases):
        if est not in eat:
            eat[est] = eoff
            ests.append(est)
            eoff += len(est)
        q[i] = (eat[est], len(est), kc if cl else 0, len(cl), 0)
        for ex in cl:
            cands[kc] = (ke, len(ex), 0, 0, 0)
            kc += 1
            for e in ex:
                exons[ke] = tuple(e)
                ke += 1
    return b"".join(ests), cands, exons, q


def expect_arrays(answers, first_candidates):
    """answers of factorization_list() per EST -> (results, facts, exons, steps) as the entry writes them;
    first_candidates[i]: the index of EST i's first candidate in the call's table"""
    from pintron_amd import capi
    res = np.zeros(len(answers), dtype=np.dtype(capi.FLIST_RESULT_DTYPE))
    fc, ex, st = [], [], []
    for i, a in enumerate(answers):
        done = a["outcome"] == DONE
        res[i] = (a["outcome"], a["stage"], a["detail"], len(fc) if done else 0, len(a["facts"]) if done else 0) + tuple(a["counts"])
        for f in a["facts"]:
            fc.append((len(ex), len(f["exons"]), f["n_merged"], int(first_candidates[i]) + f["candidate"], f["total_edit"], f["flags"]))
            ex += f["exons"]
            st += f["steps"]
    return (res, np.array(fc, dtype=np.dtype(capi.FLIST_FACT_DTYPE)).reshape(-1),
            np.array(ex, dtype=np.dtype(capi.FACTOR_DTYPE)).reshape(-1), np.array(st, dtype=np.uint8))


def same_arrays(got, want):
    return all(g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes() for g, w in zip(got, want))


# ---- hand-made cases ---------------------------------------------------------------------------------------------------
HAND_LEN = 30_000
_ACGT = np.frombuffer(b"ACGT", np.uint8)


def _layout(at, lens, introns):
    out, g = [], at
    for k, n in enumerate(lens):
        out.append((g, g + n - 1))
        g += n + (introns[k] if k < len(introns) else 0)
    return out


# the loci of the hand-made cases: (first genomic position, exon lengths, introns)
LOCI = {"main": (1000, [80, 90, 100, 85], [300, 400, 350]), "short_head": (4000, [24, 90, 100, 85], [300, 400, 350]),
        "short_tail": (7000, [80, 90, 100, 26], [300, 400, 350]), "single": (10000, [200], []),
        "gappy": (12000, [30, 120, 150, 90], [300, 400, 350]), "wide": (15000, [200, 96, 200], [600, 700]),
        "capgap": (21000, [80, 90, 100], [300, 400])}
PLANT = 25          # bases of the exon before (behind) copied in front of (behind) an exon, so that a longer variant of it matches


def hand_sequence():
    """30 kb, seeded; in front of the second exon of every locus lie the last PLANT bases of the first, and behind the
    second-to-last the first PLANT bases of the last: an exon grown by up to PLANT over either intron still matches the EST"""
    rng = np.random.default_rng(4712)
    g = bytearray(bytes(_ACGT[rng.integers(0, 4, HAND_LEN)]))
    for name, (at, lens, introns) in LOCI.items():
        x = _layout(at, lens, introns)
        if len(x) >= 3:
            g[x[1][0] - PLANT:x[1][0]] = g[x[0][1] - PLANT + 1:x[0][1] + 1]
            g[x[-2][1] + 1:x[-2][1] + 1 + PLANT] = g[x[-1][0]:x[-1][0] + PLANT]
    return bytes(g)


def locus(g, name, gaps=None):
    """(est, exons) of a locus: the exons copied from g one behind the other; gaps[k]: random bytes between exon k and k + 1,
    or ("ends", n): the first n // 2 and the last n - n // 2 bytes of the intron there"""
    at, lens, introns = LOCI[name]
    rng = np.random.default_rng(at)
    est, exons = bytearray(b"ACGTTGCAAC"), []
    for k, (a, b) in enumerate(_layout(at, lens, introns)):
        exons.append((len(est), len(est) + b - a, a, b))
        est += g[a:b + 1]
        if gaps and k < len(gaps) and gaps[k]:
            if isinstance(gaps[k], tuple):
                n = gaps[k][1]
                est += g[b + 1:b + 1 + n // 2] + g[b + 1 + introns[k] - (n - n // 2):b + 1 + introns[k]]
            else:
                est += bytes(_ACGT[rng.integers(0, 4, gaps[k])])
    est += b"TTGACCA"
    return bytes(est), exons


def ts(e, k):
    """the exon without its first k bases (k < 0: grown by -k)"""
    return (e[0] + k, e[1], e[2] + k, e[3])


def te(e, k):
    """the exon without its last k bases (k < 0: grown by -k)"""
    return (e[0], e[1] - k, e[2], e[3] - k)


def hand_cases():
    """[(name, est, [candidate], prm, tags the case was built for)] over hand_sequence()"""
    g = hand_sequence()
    out = []

    def add(name, est, cands, want=(), **kw):
        out.append((name, est, [list(c) for c in cands], params(**kw), tuple(want)))

    est, (a, b, c, d) = locus(g, "main")
    A = [a, b, c, d]
    add("one_candidate", est, [A])
    add("no_candidate", est, [], ["no_candidate"])
    # equal lists: the second widens the first
    add("widen_head", est, [[ts(a, 12), b, c, d], A], ["list_-2", "widen_head", "cfr_-2", "cfr_-1", "cfr_0"])
    add("widen_tail", est, [[a, b, c, te(d, 12)], A], ["list_-2", "widen_tail"])
    add("widen_both", est, [[ts(a, 12), b, c, te(d, 9)], A], ["list_-2", "widen_both"])
    add("equal_no_widening", est, [A, [ts(a, 12), b, c, te(d, 9)]], ["list_-2"])
    # contained, containing, different
    add("contained", est, [A, [b, c, d]], ["list_-1", "cfr_2_match"])
    add("containing", est, [[b, c, d], A], ["list_1", "removal_then_append"])
    add("contained_front", est, [A, [a, b, c]], ["list_-1", "cfr_1_match"])
    add("different", est, [[a, b], [c, d]], ["list_0", "done_2_or_more", "f1_noop", "f3_noop"])
    add("different_three", est, [[a, b], [c, d], [b, c]], ["list_0", "done_2_or_more"])
    # max_number_of_factorizations at n and at n + 1
    add("max_number_2_of_2", est, [[a, b], [c, d]], ["max_number_at"], max_number_of_factorizations=2)
    add("max_number_1_of_2", est, [[a, b], [c, d]], ["max_number_above"], max_number_of_factorizations=1)
    # the cfr_type 2 walk: the shorter list's first exon begins in front of the longer list's second one
    add("cfr_2_unconf", est, [A, [ts(b, -22), c, d]], ["cfr_2_unconf", "list_0"])
    add("cfr_2_walked", est, [A, [ts(b, -15), c, d]], ["cfr_2_walked", "list_-1"])
    est2, (a2, b2, c2, d2) = locus(g, "short_head")
    add("cfr_2_tot", est2, [[a2, b2, c2, d2], [ts(b2, -18), c2, d2]], ["cfr_2_tot", "list_0"])
    # the cfr_type 1 walk: the shorter list's last exon ends behind the longer list's second-to-last one
    add("cfr_1_unconf", est, [A, [a, b, te(c, -22)]], ["cfr_1_unconf", "list_0"])
    add("cfr_1_walked", est, [A, [a, b, te(c, -15)]], ["cfr_1_walked", "list_-1"])
    est3, (a3, b3, c3, d3) = locus(g, "short_tail")
    add("cfr_1_tot", est3, [[a3, b3, c3, d3], [a3, b3, te(c3, -15)]], ["cfr_1_tot", "list_0"])
    # a removal in front of a stop: S lies in T but not in X, and X equals T
    S, X = [ts(b, 10), c, d], [a, ts(b, 40), c, d]
    add("removal_then_stop", est, [S, X, A], ["removal_then_stop", "list_1", "list_-2", "list_0"], max_gaplength_diff=-1)
    add("stop_then_contained", est, [X, S, A], ["list_-2"], max_gaplength_diff=-1)
    # one-exon pairs
    est1, (x,) = locus(g, "single")
    add("one_equal", est1, [[x], [x]], ["one_-2"])
    add("one_inside", est1, [[x], [ts(x, 20)]], ["one_-1"])
    add("one_around", est1, [[ts(x, 20)], [x]], ["one_1", "removal_then_append"])
    add("one_apart", est1, [[te(x, 100)], [ts(x, 100)]], ["one_0"], max_coverage_diff=1.0)
    estw, (aw, bw, cw) = locus(g, "wide")
    add("one_against_list", estw, [[aw], [aw, bw, cw]], ["list_0"], max_coverage_diff=1.0)
    # FILTER 1: the relative and the absolute condition; FILTER 3 on, removing, and off
    add("f1_diff", est, [[a, b], [b, c, d]], ["f1_diff", "list_0"])
    add("f1_abs", est, [[a, b], [b, c, d]], ["f1_abs", "list_0"], max_coverage_diff=1.0)
    add("f1_noop", est, [[a, b, c], [b, c, d]], ["f1_noop", "list_0"])
    est4, (a4, b4, c4, d4) = locus(g, "gappy", gaps=[60])
    G1, G2, G3 = [a4, b4, c4, d4], [b4, ts(c4, 60), d4], [b4, te(c4, 60), d4]
    add("f3_removed", est4, [[b4, c4, d4], G2], ["f3_removed", "list_0"])
    add("f3_noop", est4, [G1, G2, G3], ["f3_noop"], max_coverage_diff=1.0)
    add("f3_off", est4, [G1, G2, G3], ["f3_off", "gaps_drop_one"], max_coverage_diff=1.0, max_gaplength_diff=-1)
    add("gaps_drop_all", est4, [G1], ["gaps_drop_all"], max_gaplength_diff=-1)
    add("max_number_behind_filter_4", est4, [G1, G2, G3], ["max_number_at", "gaps_drop_one"], max_coverage_diff=1.0,
        max_gaplength_diff=-1, max_number_of_factorizations=2)
    # dropped_first in one entry of two: a first exon of 22 bases whose bases also lie in front of the second exon (planted),
    # so the refinement of the first intron takes it into the second, and :476-485 drop it; the other entry begins at b
    a_s = ts(a, a[1] - a[0] + 1 - 22)
    other = [b, ts(c, 60), d]
    add("dropped_first_one_of_two", est, [[a_s, b, c, d], other], ["dropped_one_of_two", "list_0"], max_coverage_diff=1.0,
        max_gaplength_diff=-1)
    add("dropped_first_second_of_two", est, [other, [a_s, b, c, d]], ["dropped_one_of_two"], max_coverage_diff=1.0, max_gaplength_diff=-1)
    # a filtered entry that would have met the gaps cap: B has an EST gap of 65, A closes it; unequal under max_site_difference 3
    est5, (a5, b5, c5) = locus(g, "capgap", gaps=[("ends", 65)])
    A5 = [(a5[0], a5[1] + 32, a5[2], a5[3] + 32), (b5[0] - 33, b5[1], b5[2] - 33, b5[3]), c5]
    add("filtered_before_cap", est5, [A5, [a5, b5, c5]], ["filtered_before_cap", "f3_removed"], max_site_difference=3)
    add("gaps_cap_alone", est5, [[a5, b5, c5]], ["host_3_1"])
    add("gaps_cap_second", est5, [A5, [a5, b5, c5]], ["host_3_1"], max_site_difference=3, max_gaplength_diff=-1)
    # HOST at stage 1 from a candidate that is not the first; the lowest index decides between a refused input and a cap
    bad = [c, (d[0], len(est) + 1, d[2], d[3])]
    add("refused_second", est, [[a, b], bad], ["host_1_2"])
    add("refused_first_of_two_bad", est, [bad, [a, b], [ts(b, 3)] + [(b[0] + 4 + k, b[0] + 4 + k, b[2] + 4 + k, b[2] + 4 + k) for k in range(64)]],
        ["host_1_2"])
    add("cap_first_of_two_bad", est, [[ts(b, 3)] + [(b[0] + 4 + k, b[0] + 4 + k, b[2] + 4 + k, b[2] + 4 + k) for k in range(64)], bad], ["host_1_1"])
    return g, out


def generated_cases(g):
    """lists most of which end DONE with two or more factorizations, made rather than searched (the real records alone give fewer
    than tests/test_flists_cpu.py asks for): pairs and triples of partial candidates that differ, at four loci, with the
    outer ends trimmed by k"""
    out = []
    for name in ("main", "short_head", "short_tail", "gappy"):
        est, (a, b, c, d) = locus(g, name)
        for k in range(4):
            a_k, d_k = ts(a, k), te(d, 2 * k)
            out.append(("generated/%s_pair_%d" % (name, k), est, [[a_k, b, c], [b, c, d_k]], DEFAULTS, ()))
            out.append(("generated/%s_triple_%d" % (name, k), est, [[a_k, b, c], [b, c, d_k], [ts(b, 5 + k), c, d_k], [a_k, b]],
                        params(max_coverage_diff=1.0, max_gaplength_diff=-1 if k & 1 else 20), ()))
    return out


def fact_hand_as_lists():
    """fact_lib's hand-made cases (HOST at the stages of one candidate, the caps' last accepted values) over fact_lib's own
    sequence, each as a list of one candidate: (genomic, [(name, est, [candidate], prm, ())])"""
    fg, fcases = FL.hand_cases()
    out = []
    for name, est, exons, prm, want in fcases:
        out.append(("fact/" + name, est, [list(exons)] if exons else [], tuple(prm) + DEFAULTS[5:], ()))
    return fg, out


def cap_cases(g):
    """64 and 65 candidates of one exon each, constructed: pairwise apart on the genomic sequence, so all are listed"""
    at, n, w = 18000, 200, 120
    est = b"ACGTTGCAAC" + g[at:at + n] + b"TTGACCA"
    cands = [[(10 + k, 10 + k + w - 1, at + k, at + k + w - 1)] for k in range(65)]       # staggered windows: none inside another
    return [("cands_64", est, cands[:64], DEFAULTS, ("cands_64", "one_0", "done_2_or_more")), ("cands_65", est, cands, DEFAULTS, ("cands_65",))]


# ---- the host's ef_chain_factorizations ----------------------------------------------------------------------------------
class Host:
    def __init__(self, genomic: bytes):
        import ctypes as C
        import struct
        import cand_lib as KL
        H = self.H = KL.host_lib()
        H.ef_gpu_open.restype = C.c_void_p
        H.ef_gpu_open.argtypes = [C.c_void_p]
        H.ef_gpu_close.argtypes = [C.c_void_p]
        H.ef_chain_factorizations.restype = C.c_uint
        H.ef_chain_factorizations.argtypes = [C.c_char_p, C.c_void_p, C.c_char_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                              C.c_void_p, C.c_size_t, C.POINTER(C.c_uint), C.POINTER(C.c_uint)]
        H.ef_chain_factorizations_from.restype = C.c_uint
        H.ef_chain_factorizations_from.argtypes = [C.c_void_p, C.c_void_p, C.c_uint, C.c_void_p, C.c_char_p, C.c_void_p, C.c_void_p,
                                                   C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint),
                                                   C.POINTER(C.c_uint)]
        H.ef_config_set_chain_settings.argtypes = [C.c_void_p, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_uint,
                                                   C.c_int, C.c_int]
        self.gen = C.create_string_buffer(genomic, len(genomic) + 2)
        self.seq = C.create_string_buffer(4096)
        struct.pack_into("<QQQ", self.seq, 0, 0, C.addressof(self.gen), C.addressof(self.gen))
        self.cfg = C.create_string_buffer(4096)
        H.ef_config_defaults(self.cfg)
        self.be = H.ef_gpu_open(self.seq)
        assert self.be

    def _configure(self, prm, L=15):
        import struct
        self.H.ef_config_defaults(self.cfg)
        struct.pack_into("<I", self.cfg, 0, L)
        self.H.ef_config_set_chain_settings(self.cfg, float(prm[0]), int(prm[1]), int(prm[2]), int(prm[3]), int(prm[4]), float(prm[5]),
                                            int(prm[6]), int(prm[7]), int(prm[8]))

    def _call(self, fn, *head):
        import ctypes as C
        ecap, fcap = 8192, 512
        ex = (C.c_int32 * (4 * ecap))()
        first = (C.c_uint * (fcap + 1))()
        nf, ne = C.c_uint(0), C.c_uint(0)
        kind = fn(*head, self.gen, self.be, ex, ecap, first, fcap, C.byref(nf), C.byref(ne))
        assert nf.value <= fcap and ne.value <= ecap
        return kind, [[tuple(ex[4 * k:4 * k + 4]) for k in range(first[f], first[f + 1])] for f in range(nf.value)]

    def factorizations(self, rec, est: bytes, L=15, prm=DEFAULTS):
        """ef_chain_factorizations on one record under prm (min_intron_length is the enumeration's too):
        (0 flagged | 1 none | 2, [[exon]])"""
        self._configure(prm, L)
        return self._call(self.H.ef_chain_factorizations, rec, self.cfg, est)

    def from_candidates(self, est: bytes, cands, prm=DEFAULTS):
        """ef_chain_factorizations_from on candidates [[exon]]: (1 none | 2, [[exon]])"""
        import ctypes as C
        self._configure(prm)
        flat = [v for c in cands for e in c for v in e]
        ex = (C.c_int32 * max(1, len(flat)))(*flat)
        first = (C.c_uint * (len(cands) + 1))(*np.cumsum([0] + [len(c) for c in cands]).tolist())
        return self._call(self.H.ef_chain_factorizations_from, ex, first, len(cands), self.cfg, est)

    def close(self):
        self.H.ef_gpu_close(self.be)


def agrees_with_host(ans, host_answer):
    """the restatement's answer against ef_chain_factorizations': HOST says nothing (the host has no caps)"""
    kind, lists = host_answer
    if ans["outcome"] == HOST:
        return True
    if ans["outcome"] == EMPTY:
        return kind == 1
    return kind == 2 and lists == [f["exons"] for f in ans["facts"]]


# ---- the fixture ---------------------------------------------------------------------------------------------------------
_fixture = []


def load_fixture():
    """({name: genomic}, [case], counts): a case is dict(name, seq, est, cands, prm, tags, answer); computed once, shared: do
    not modify.  The sequences are candidates.json.gz's, hand_sequence() ("hand") and fact_lib's ("fact")."""
    if not _fixture:
        import cand_lib as KL
        with gzip.open(FIXTURE, "rt") as f:
            doc = json.load(f)
        seqs = dict(KL.load_fixture()[0])
        seqs.update({"hand": hand_sequence(), "fact": FL.hand_sequence()})
        ests = [e.encode() for e in doc["ests"]]
        cases = []
        for name, seq, est, cands, prm, tags, a in doc["cases"]:
            ans = answer(a[0], a[1], a[2], a[3], [dict(candidate=f[0], exons=[tuple(e) for e in f[1]], steps=f[2], n_merged=f[3],
                                                        total_edit=f[4], flags=f[5]) for f in a[4]])
            cases.append(dict(name=name, seq=seq, est=ests[est], cands=[[tuple(e) for e in x] for x in cands], prm=tuple(prm), tags=tags,
                              answer=ans))
        _fixture.append((seqs, cases, doc["counts"]))
    return _fixture[0]


def real_ests():
    """{(source, set name): [EST]} of the real inputs behind candidate_lists.json.gz's `real/<set>/<k>`, `path/...` and
    `empty/...` cases: EST k of that run; computed once"""
    if not _real:
        import cand_lib as KL
        import meg_lib as M
        for src, (gfa, efa) in KL.real_inputs().items():
            for set_name, prm in KL.fixture_sets():
                exp, _ = M.first_attempt_megs(gfa, efa, prm)
                _real[(src, set_name)] = [e["seq"] if isinstance(e["seq"], bytes) else e["seq"].encode() for e in exp]
    return _real


_real = {}


def real_case(c):
    """a case of enum_lib's fixture that comes from a real input -> (est, [candidate], prm), or None"""
    parts = c["name"].split("/")
    if len(parts) != 3 or c["seq"] == "hand" or c["kind"] != 3:
        return None
    est = real_ests()[(c["seq"], parts[1])][int(parts[2])]
    return est, [[tuple(e) for e in ex] for _, _, ex in c["cands"]], params(min_intron_length=c["min_intron"])


def answer_to_json(a):
    return [a["outcome"], a["stage"], a["detail"], list(a["counts"]),
            [[f["candidate"], [list(e) for e in f["exons"]], f["steps"], f["n_merged"], f["total_edit"], f["flags"]] for f in a["facts"]]]
