"""CPU restatement of pgpu_index_small_chains: the last two routines of refine_EST_factorizations that concern one
factorization alone -- search_for_new_small_exons (src/factorization-refinement.c:875-912, with search_small_exon_at_prefix
:500-606 and search_small_exon :641-871) and clean_factorizations (:914-950).

small           the three steps in Python, lists and loops as the reference writes them, over an `ops` object that answers
                the device questions (common factor, edit distance, border refinement, intron class, small-exon search,
                banded distance): OracleOps asks tests/oracle_lib.py and tests/small_exon_lib.py; the caps of the entry.
einval          the PGPU_EINVAL rules of the entry for one call (tail_lib's, and the parameters).
make_world      hand-made cases over a seeded sequence of a few kilobases per locus, one builder per group of tags.
generated       fresh ordinary factorizations over a world's loci, read only (the GPU test's 2 000).
batch_arrays / expect_arrays   the arrays of the entry for a batch and for its answers.
device_route    today's route on the device: the same questions as PGPU_DP_LCF, PGPU_DP_ED, PGPU_DP_BORDERS and
                PGPU_DP_KBAND jobs of DP plans plus pgpu_index_classify and pgpu_index_small_exons, one round of each per
                pass, the glue of small() on the host.
load_fixture    tests/golden/small_chains.json.gz (tools/make_small_golden.py).
"""
import gzip
import json
import os

import numpy as np

import clean_lib as CL
import refine_lib as RL
import oracle_lib as O
import small_exon_lib as SE
import tail_lib as TL

FIXTURE = os.path.join(RL.ROOT, "tests", "golden", "small_chains.json.gz")
OK, ERANGE, EINVAL = 0, -34, -22
MAX_EXONS = 64            # PGPU_SMALL_MAX_EXONS
MAX_PREFIX_WINDOW = 256   # PGPU_SMALL_MAX_PREFIX_WINDOW
MAX_KBAND = 31            # PGPU_SMALL_MAX_KBAND
LB, UB, MPB = 6, 23, 6    # _LB_SMALL_EXON_LENGTH_, _UB_SMALL_EXON_LENGTH_, _MIN_PERFECT_BORDER_LENGTH_
STEP_PREFIX, STEP_BETWEEN, STEP_MOVED, STEP_NOISY, STEP_EXTERNAL = 1, 2, 4, 16, 32
REF_EXONS, REF_WINDOW, REF_LCF, REF_KBAND, REF_ORDER = 1, 2, 3, 4, 5

# the cover of the fixture (tools/make_small_golden.py asks for MIN_PER_TAG cases of each)
TAGS = ("est_start_6", "est_start_7", "gate_28", "gate_29", "cflen_5", "cflen_6", "lcf_tie_gen", "lcf_tie_est",
        "est_start_46", "est_start_47", "prefix_equal", "prefix_ed", "prefix_borders_no", "intron_short_by_1",
        "mil_not_positive", "not_canonical", "lower_gtag", "mixed_gtag", "offp_below_6", "offp_wraps", "window_256", "window_257",
        "piece_one_n", "piece_two_n", "at_first_bad", "past_first_bad", "prefix_added",
        "pair_gate_51", "pair_gate_52", "e1slen_by_gen", "dist_2", "dist_3", "class2_dist_0", "extension",
        "gate_f1", "gate_f2", "gate_room", "gate_elen", "search_none", "search_tie", "winner_6", "three_insertions",
        "grow_past_64", "exons_65", "efact_n", "between_added",
        "noisy_middle_tie", "kband_31", "kband_32", "end_9", "end_10", "end_19", "end_20", "end_site_ok", "end_no_donor",
        "end_no_acceptor", "end_differs", "emptied_noisy", "emptied_external", "orig_decides", "inserted_dropped",
        "disordered")
# (a lower-case gt .. ag IN FRONT of the first exon puts that exon behind the first byte that is no upper-case ACGT, refused =
# 3; but the intron step 1 tests lies in G[pg .. min(GEN_end + 1, GEN_start + 23)) and may begin AT GEN_start: `lower_gtag`
# and `mixed_gtag` are such cases, an exon laid over a short intron and the true exon behind it)
MIN_PER_TAG = 3
REFUSED_TAGS = ("window_257", "piece_two_n", "past_first_bad", "exons_65", "kband_32", "disordered")


def first_bad(gen: bytes) -> int:
    """position of the first byte that is no upper-case A, C, G or T (the length when there is none)"""
    for i, c in enumerate(gen):
        if c not in b"ACGT":
            return i
    return len(gen)


class OracleOps:
    """the questions, answered by the CPU oracle and the pinned restatements; one object per sequence"""

    def __init__(self, gen: bytes):
        self.gen = gen
        self.first_bad = first_bad(gen)
        self._cls = None

    def lcf_prefix(self, gstart: int, piece: bytes):
        r = O.lcf(self.gen[:gstart], piece)
        return r["len"], r["occ1"], r["occ2"]

    def ed(self, a: bytes, b: bytes):
        return O.edit_distance(a, b)

    def borders(self, p: bytes, gstart: int, glen: int, p0: int, p1: int, max_errs: int):
        gend = gstart + glen
        return O.refine_borders(p, self.gen[gstart:gend], p0, p1, max_errs, self.gen[gend:gend + 2])

    def lcf(self, a: bytes, b: bytes):
        r = O.lcf(a, b)
        return r["len"], r["occ1"], r["occ2"]

    def classify(self, start: int, end: int):
        if self._cls is None:
            self._cls = SE.Classifier(self.gen)
        return self._cls.classify(start, end)

    def sexon(self, efact: bytes, allgstart, allglen, f1slen, f2plen, mil, info=None):
        if info is not None:
            info["_ties"] = _search_ties(self.gen, efact, allgstart, allglen, f1slen, f2plen, mil, self.classify)
        return SE.search_small_exon_loop(self.gen, efact, allgstart, allglen, f1slen, f2plen, mil, self.classify)[:4]

    def kband(self, g: bytes, e: bytes, ub: int) -> bool:
        return bool(O.kband(g, e, ub)["ok"])


def _search_ties(gen, efact, allgstart, allglen, f1slen, f2plen, mil, classify):
    """how many candidates of the winning length the loop of :772-834 meets (the tag's cost: a second search)"""
    best = SE.search_small_exon_loop(gen, efact, allgstart, allglen, f1slen, f2plen, mil, classify)
    if best[0] < LB:
        return 0
    elen, n = len(efact), 0
    allgfact = gen[allgstart:allgstart + allglen]
    for offstart in range(min(f1slen + 1 - 6, elen + 1 - 6, allglen + 1 - 2 * mil - 6)):
        offend = elen - offstart - best[0]
        if not 0 <= offend < min(f2plen + 1 - 6, elen + 1 - offstart - 6, allglen + 1 - 2 * mil - 6 - offstart):
            continue
        pat = efact[offstart:elen - offend]
        occ = allgfact.find(pat, offstart + mil, allglen - offend - mil)
        while occ >= 0:
            if classify(allgstart + offstart, allgstart + occ - 1) != 2 and \
                    classify(allgstart + occ + len(pat), allgstart + allglen - offend - 1) != 2:
                n += 1
            occ = allgfact.find(pat, occ + 1, allglen - offend - mil)
    return n


class _Refuse(Exception):
    def __init__(self, code, why):
        Exception.__init__(self, why)
        self.code = code


def _ed(ops, a, b, info):
    """compute_edit_distance (src/compute-alignments.c:240-249): 0 without a dynamic program for equal strings"""
    if a == b:
        return 0
    info["dp_ed"] = info.get("dp_ed", 0) + 1
    return ops.ed(a, b)


def _lcf_ties(gen_prefix: bytes, piece: bytes, cflen: int):
    """(more than one start in the sequence, more than one start in the piece) among the factors of the longest length;
    exact matching (the tag is asked for pieces without an N)"""
    gs, es = set(), set()
    for pe in range(len(piece) - cflen + 1):
        at = gen_prefix.find(piece[pe:pe + cflen])
        if at >= 0:
            es.add(pe)
            while at >= 0:
                gs.add(at)
                at = gen_prefix.find(piece[pe:pe + cflen], at + 1)
    return len(gs) > 1, len(es) > 1


def prefix_search(est: bytes, gen: bytes, p1, mil: int, ops, info):
    """search_small_exon_at_prefix (:500-606) -> the new exon or None; p1 (a list) is moved"""
    e1len, g1len = p1[1] + 1 - p1[0], p1[3] + 1 - p1[2]
    info["gate_28"] = e1len + p1[0] == LB + UB - 1
    info["gate_29"] = e1len + p1[0] == LB + UB
    if e1len + p1[0] < LB + UB:
        return None
    eplen = min(p1[0], p1[2], 2 * UB)
    epfact = est[p1[0] - eplen:p1[0]]
    cflen = pg = pe = 0
    if eplen:
        odd = [c for c in epfact if c not in b"ACGT"]
        wild = [c for c in odd if c in b"Nn"]
        if p1[2] > ops.first_bad and not info.get("no_caps"):
            info["past_first_bad"] = p1[2] == ops.first_bad + 1
            raise _Refuse(REF_LCF, "a genomic prefix with a byte outside ACGT")
        if (len(odd) > len(wild) or len(wild) > 1) and not info.get("no_caps"):
            info["piece_two_n"] = len(wild) == 2 and len(odd) == 2
            raise _Refuse(REF_LCF, "an EST piece the suffix array cannot answer")
        info["piece_one_n"] = len(wild) == 1
        info["at_first_bad"] = p1[2] == ops.first_bad
        info["dp_lcf"] = info.get("dp_lcf", 0) + 1
        cflen, pg, pe = ops.lcf_prefix(p1[2], epfact)
    info["cflen_5"] = cflen == LB - 1
    info["cflen_6"] = cflen == LB
    if cflen < LB:
        return None
    if info.get("tagged") and not info["piece_one_n"]:
        info["lcf_tie_gen"], info["lcf_tie_est"] = _lcf_ties(gen[:p1[2]], epfact, cflen)
    e1plen = min(e1len, g1len, UB)
    a, b = est[p1[0]:p1[0] + e1plen], gen[p1[2]:p1[2] + e1plen]
    edp = _ed(ops, a, b, info)
    info["prefix_equal"], info["prefix_ed"] = a == b, edp > 0
    # `pe` is an offset inside epfact and an absolute EST coordinate from here on, as in the reference
    info["est_start_46"], info["est_start_47"] = p1[0] == 2 * UB, p1[0] == 2 * UB + 1
    allelen = min(p1[1] + 1, p1[0] + UB) - pe
    allglen = min(p1[3] + 1, p1[2] + UB) - pg
    if allelen < 2 * LB:
        return None
    if allelen > MAX_PREFIX_WINDOW and not info.get("no_caps"):
        info["window_257"] = allelen == MAX_PREFIX_WINDOW + 1
        raise _Refuse(REF_WINDOW, "a prefix window of %d EST bytes" % allelen)
    info["window_256"] = allelen == MAX_PREFIX_WINDOW
    info["dp_borders"] = info.get("dp_borders", 0) + 1
    r = ops.borders(est[pe:pe + allelen], pg, allglen, LB, allelen - LB, edp)
    if not r["ok"]:
        info["prefix_borders_no"] = True
        return None
    off_p, off_t1, off_t2 = r["off_p"], r["off_t1"], r["off_t2"]
    info["mil_not_positive"] = mil <= 0
    if off_t2 - off_t1 < mil:
        info["intron_short_by_1"] = off_t2 - off_t1 == mil - 1
        return None
    s, e = pg + off_t1, pg + off_t2 - 1
    if not (s >= 0 and s + 1 < len(gen) and e >= 1 and e < len(gen)):
        info["outside"] = True                               # the reference reads outside the sequence here
        return None
    pair = (gen[s:s + 2], gen[e - 1:e + 1])
    if pair not in ((b"GT", b"AG"), (b"gt", b"ag")):
        info["not_canonical"] = True
        if (pair[0].upper(), pair[1].upper()) == (b"GT", b"AG"):
            info["mixed_gtag"] = True
        return None
    info["lower_gtag"] = pair == (b"gt", b"ag")
    if off_p < pe:
        info["offp_wraps"] = True                            # unsigned: a huge value, not below 6
    elif off_p - pe < LB:
        info["offp_below_6"] = True
        return None
    new = (pe, pe + off_p - 1, pg, pg + off_t1 - 1)
    p1[0], p1[2] = pe + off_p, pg + off_t2
    info["prefix_added"] = True
    return new


def between_search(est: bytes, gen: bytes, p1, p2, mil_raw: int, ops, info):
    """search_small_exon (:641-871) -> the new exon or None; p1 and p2 (lists) are moved"""
    e1len, g1len = p1[1] + 1 - p1[0], p1[3] + 1 - p1[2]
    e2len, g2len = p2[1] + 1 - p2[0], p2[3] + 1 - p2[2]
    if e1len + e2len == LB + 2 * UB - 1:
        info["pair_gate_51"] = True
    if e1len + e2len == LB + 2 * UB:
        info["pair_gate_52"] = True
    if e1len + e2len < LB + 2 * UB:
        return None
    e1slen = min(e1len, g1len, UB)
    if g1len < min(e1len, UB):
        info["e1slen_by_gen"] = True
    e1sstart, g1sstart = p1[1] + 1 - e1slen, p1[3] + 1 - e1slen
    e2plen = min(e2len, g2len, UB)
    e2pstart, g2pstart = p2[0], p2[2]
    e1s, g1s = est[e1sstart:e1sstart + e1slen], gen[g1sstart:g1sstart + e1slen]
    e2p, g2p = est[e2pstart:e2pstart + e2plen], gen[g2pstart:g2pstart + e2plen]
    sed, ped = _ed(ops, e1s, g1s, info), _ed(ops, e2p, g2p, info)
    info["dp_class"] = info.get("dp_class", 0) + 1
    cls = ops.classify(p1[3] + 1, p2[2] - 1)
    if sed + ped == 2 and cls != 2:
        info["dist_2"] = True
    if sed + ped == 3:
        info["dist_3"] = True
    if not (sed + ped > 2 or cls == 2):
        return None
    if sed + ped == 0:
        info["class2_dist_0"] = True
    f1slen, e1socc, g1socc = e1slen, 0, 0
    if sed > 0:
        info["dp_lcf_small"] = info.get("dp_lcf_small", 0) + 1
        f1slen, e1socc, g1socc = ops.lcf(e1s, g1s)
    f2plen, e2pocc, g2pocc = e2plen, 0, 0
    if ped > 0:
        info["dp_lcf_small"] = info.get("dp_lcf_small", 0) + 1
        f2plen, e2pocc, g2pocc = ops.lcf(e2p, g2p)
    if f1slen == e1slen and e2pocc > 0:                      # :725-737: the EST byte does not move
        nf = f1slen + 1
        while nf - f1slen < e2pocc and est[e1sstart + e1socc + f1slen] == gen[g2pstart + nf - f1slen]:
            nf += 1
        if nf - 1 > f1slen:
            f1slen = nf - 1
            info["extension"] = True
    elen = (e1slen - e1socc) + (e2pocc + f2plen) - 2 * MPB
    estart = e1sstart + e1socc + MPB
    allgstart = g1sstart + g1socc + MPB
    allglen = g2pstart + g2pocc + f2plen - MPB - allgstart
    mil = max(4, mil_raw)
    closed = [f1slen < MPB, f2plen < MPB, allglen < 2 * mil + LB, elen < LB]
    if sum(closed) == 1:
        info[("gate_f1", "gate_f2", "gate_room", "gate_elen")[closed.index(True)]] = True
    if elen < 0 and f1slen >= MPB and f2plen >= MPB:
        info["outside"] = True                               # the reference's unsigned length wraps and its copy leaves the EST
    if any(closed) or elen < LB or allglen <= 0 or allgstart + allglen > len(gen):
        return None
    efact = est[estart:estart + elen]
    if any(c in b"Nn" for c in efact):
        info["efact_n"] = True
    info["dp_sexon"] = info.get("dp_sexon", 0) + 1
    ln, os_, oe, gpos = ops.sexon(efact, allgstart, allglen, f1slen, f2plen, mil, info if info.get("tagged") else None)
    if info.get("tagged") and info.pop("_ties", 0) > 1:
        info["search_tie"] = True
    if ln < LB:
        info["search_none"] = True
        return None
    if ln == LB:
        info["winner_6"] = True
    new = (estart + os_, estart + os_ + ln - 1, gpos, gpos + ln - 1)
    p1[1], p1[3] = estart + os_ - 1, allgstart + os_ - 1
    p2[0], p2[2] = estart + os_ + ln, allgstart + allglen - oe
    info["between_added"] = True
    return new


def _external_ok(seq: bytes, gen: bytes, ex, end, info):
    """clean_external_exons (:1706-1825) on the head (end 0) or the tail (end 1) of the run `ex`"""
    x = ex[0] if end == 0 else ex[-1]
    n = x[3] - x[2] + 1
    for k in (9, 10, 19, 20):
        if n == k:
            info["end_%d" % k] = True
    ok = n >= 10
    if ok and n < 20:
        up, at = CL.upper, CL.byte_at
        if end == 0:
            donor = up(at(gen, x[3] + 1)) == 71 and up(at(gen, x[3] + 2)) in (84, 67)
            acceptor = len(ex) > 1 and up(at(gen, ex[1][2] - 2)) == 65 and up(at(gen, ex[1][2] - 1)) == 71
        else:
            acceptor = up(at(gen, x[2] - 2)) == 65 and up(at(gen, x[2] - 1)) == 71
            donor = len(ex) > 1 and up(at(gen, ex[-2][3] + 1)) == 71 and up(at(gen, ex[-2][3] + 2)) in (84, 67)
        if len(ex) > 1 and not donor:
            info["end_no_donor"] = True
        if len(ex) > 1 and donor and not acceptor:
            info["end_no_acceptor"] = True
        ok = len(ex) > 1 and donor and acceptor
        if ok and CL.sub(gen, x[2], x[3]) != CL.sub(seq, x[0], x[1]):
            info["end_differs"] = True
            ok = False
        if ok:
            info["end_site_ok"] = True
    return ok


def last_cleaning(seq: bytes, gen: bytes, ex, steps, ops, info, external_first=False):
    """clean_factorizations (:914-950) on `seq` -> (verdict, first_kept, n_kept); the steps get their bits"""
    if any(e[2] <= e[3] and CL.max_edit(e[3] - e[2] + 1) > MAX_KBAND for e in ex) and not info.get("no_caps"):
        info["kband_32"] = max(CL.max_edit(e[3] - e[2] + 1) for e in ex if e[2] <= e[3]) == MAX_KBAND + 1
        raise _Refuse(REF_KBAND, "a bound beyond the K-band on the lanes")
    if any(e[2] <= e[3] and CL.max_edit(e[3] - e[2] + 1) == MAX_KBAND for e in ex):
        info["kband_31"] = True
    lo, hi = 0, len(ex)

    def noisy():
        nonlocal lo, hi
        bad = []
        for i in range(lo, hi):
            e = ex[i]
            ok = False
            if e[2] <= e[3]:
                info["dp_kband"] = info.get("dp_kband", 0) + 1
                ok = ops.kband(CL.sub(gen, e[2], e[3]), CL.sub(seq, e[0], e[1]), CL.max_edit(e[3] - e[2] + 1))
            if not ok:
                steps[i] |= STEP_NOISY
                bad.append(i - lo + 1)
        tie = {}
        run = CL.best_run([tuple(e) + (i,) for i, e in enumerate(ex)][lo:hi], bad, tie)
        if bad and tie.get("tie") and any(lo < lo + b - 1 < hi - 1 for b in bad):
            info["noisy_middle_tie"] = True
        lo, hi = (run[0][4], run[-1][4] + 1) if run else (lo, lo)
        return lo == hi

    def external():
        nonlocal lo, hi
        for end in (0, 1):
            if lo == hi:
                return True
            if not _external_ok(seq, gen, ex[lo:hi], end, info):
                steps[lo if end == 0 else hi - 1] |= STEP_EXTERNAL
                if end == 0:
                    lo += 1
                else:
                    hi -= 1
        return lo == hi

    order = ((external, 2), (noisy, 1)) if external_first else ((noisy, 1), (external, 2))
    for step, verdict in order:
        if step():
            info["emptied_noisy" if verdict == 1 else "emptied_external"] = True
            return verdict, 0, 0
    return 0, lo, hi - lo


def small(orig: bytes, est: bytes, gen: bytes, exons, mil: int, ops=None, info=None, again=False, clean_on_working=False,
          external_first=False):
    """One query -> (status, refused, verdict, prefix_added, n_added, n_list, first_kept, n_kept, the list, its steps).
    exons: [(EST_start, EST_end, GEN_start, GEN_end)], a query the entry accepts (einval).  `info` (a dict) receives what the
    fixture's cover counts; info["tagged"] asks for the tags that cost a second computation, info["no_caps"] lifts the caps
    of the entry (the host code has none).  The three last arguments break the restatement on purpose
    (tools/make_small_golden.py: the fixture must notice): an inserted exon is analysed again, step 3 runs on the working
    sequence, step 3 runs in clean_chains' order."""
    info = {} if info is None else info
    ops = OracleOps(gen) if ops is None else ops
    given = [tuple(int(v) for v in e) for e in exons]
    n = len(given)

    def refusal(code):
        return ERANGE, code, 0, 0, 0, 0, 0, 0, given, [0] * n
    if n > MAX_EXONS and not info.get("no_caps"):
        info["refused"] = "more than %d exons" % MAX_EXONS
        info["exons_65"] = n == MAX_EXONS + 1
        return refusal(REF_EXONS)
    if any(e[0] > e[1] or e[2] > e[3] for e in given) or any(a[1] >= b[0] or a[3] >= b[2] for a, b in zip(given, given[1:])):
        info["refused"] = info["disordered"] = "exons not in order"
        return refusal(REF_ORDER)
    ex = [list(e) for e in given]
    out, steps = [], []
    try:
        # ---- step 1
        p1, p1_steps = ex[0], 0
        info["est_start_6"], info["est_start_7"] = p1[0] == LB, p1[0] == LB + 1
        if p1[0] > LB:
            new = prefix_search(est, gen, p1, mil, ops, info)
            if new is not None:
                out.append(list(new))
                steps.append(STEP_PREFIX)
                p1_steps = STEP_MOVED
        prefix_added = len(out)
        # ---- step 2
        inserted = 0
        k = 1
        while k < len(ex):
            p2, p2_steps = ex[k], 0
            new = between_search(est, gen, p1, p2, mil, ops, info)
            if new is not None:
                inserted += 1
                p1_steps |= STEP_MOVED
                p2_steps = STEP_MOVED
                if again:                                        # (broken on purpose: the new exon becomes p1 of the same p2)
                    out.append(p1)
                    steps.append(p1_steps)
                    p1, p1_steps = list(new), STEP_BETWEEN
                    continue
                out.append(p1)
                steps.append(p1_steps)
                out.append(list(new))
                steps.append(STEP_BETWEEN)
            else:
                out.append(p1)
                steps.append(p1_steps)
            p1, p1_steps = p2, p2_steps
            k += 1
        out.append(p1)
        steps.append(p1_steps)
        info["three_insertions"] = inserted >= 3
        info["grow_past_64"] = n <= MAX_EXONS < len(out)
        # ---- step 3
        verdict, first, kept = last_cleaning(est if clean_on_working else orig, gen, out, steps, ops, info, external_first)
    except _Refuse as why:
        info["refused"] = str(why)
        return refusal(why.code)
    if info.get("tagged"):
        info["inserted_dropped"] = any(s & STEP_BETWEEN and not first <= i < first + kept for i, s in enumerate(steps))
        if orig != est:
            st2 = [s & ~(STEP_NOISY | STEP_EXTERNAL) for s in steps]
            info["orig_decides"] = last_cleaning(est, gen, out, st2, ops, {}) != (verdict, first, kept)
    return OK, 0, verdict, prefix_added, len(out) - n, len(out), first, kept, [tuple(e) for e in out], steps


def kept_exons(answer):
    """the exons a caller goes on with: the run step 3 keeps"""
    return answer[8][answer[6]:answer[6] + answer[7]]


def tags_of(info):
    return sorted(t for t in TAGS if info.get(t))


def einval(ests_len, gen_len, exons, queries, params_reserved=0):
    """True when pgpu_index_small_chains refuses the whole call"""
    return params_reserved != 0 or TL.einval(ests_len, gen_len, exons, queries)


# ---- worlds: loci planted in a seeded sequence ----------------------------------------------------------------------
#   [S] GT i1 AG [A] GT i2 AG [M] GT i3 AG [B] GT i4 AG [Z]
# S a small first exon, A and B ordinary exons, M a small exon between them, Z a last exon.  Everything is upper-case
# ACGT unless a builder says otherwise; the introns have their GT .. AG and no branch point is planted, so an intron
# between two true exon ends classifies as U2 and a shifted one mostly as not classified.
LOCUS = 1400


def other_base(c):
    return TL.other_base(c)


class Locus:
    def __init__(self, g: bytearray, at: int, rng, s_len=None, m_len=None, z_len=None, intr=(70, 160), a_len=None, b_len=None,
                 pad=60):
        self.g = g
        r = lambda lo, hi: int(rng.integers(lo, hi))
        self.s_len = r(8, 20) if s_len is None else s_len
        self.a_len = r(45, 80) if a_len is None else a_len
        self.m_len = r(8, 17) if m_len is None else m_len
        self.b_len = r(45, 80) if b_len is None else b_len
        self.z_len = r(25, 60) if z_len is None else z_len
        self.i = [r(*intr) for _ in range(4)]
        p = at + pad
        self.s = p
        p += self.s_len
        self.a = p + self.i[0]
        p = self.a + self.a_len
        self.m = p + self.i[1]
        p = self.m + self.m_len
        self.b = p + self.i[2]
        p = self.b + self.b_len
        self.z = p + self.i[3]
        self.end = self.z + self.z_len
        assert self.end + 40 <= at + LOCUS
        for lo, hi in ((self.s + self.s_len, self.a), (self.a + self.a_len, self.m), (self.m + self.m_len, self.b),
                       (self.b + self.b_len, self.z)):
            g[lo:lo + 2] = b"GT"
            g[hi - 2:hi] = b"AG"

    def seq(self, lo, n):
        return bytes(self.g[lo:lo + n])


class World:
    """the sequence under construction and the cases planted in it: (name, orig, est, exons, min_intron_length)"""

    def __init__(self, seed, n_loci):
        self.seed = seed
        self.rng = np.random.default_rng(seed)
        self.g = bytearray(RL.rnd(self.rng, 200 + n_loci * LOCUS))
        self.n_loci, self.used = n_loci, 0
        self.cases = []

    def locus(self, **kw):
        at = 100 + self.used * LOCUS
        self.used += 1
        assert self.used <= self.n_loci
        return Locus(self.g, at, self.rng, **kw)

    def add(self, name, est, exons, mil=60, orig=None):
        self.cases.append((name, bytes(est if orig is None else orig), bytes(est), [tuple(int(v) for v in e) for e in exons], int(mil)))


def prefix_case(L, flank=b"", s_keep=None, cut=0):
    """EST = flank + S + A, the factorization the one exon A (less its first `cut` bytes, given to nobody): the prefix
    search finds S"""
    s = L.seq(L.s, L.s_len) if s_keep is None else s_keep
    est = flank + s + L.seq(L.a, L.a_len)
    e0 = len(flank) + len(s)
    return est, [(e0 + cut, len(est) - 1, L.a + cut, L.a + L.a_len - 1)]


def between_case(L, k=None, rng=None, lead=b""):
    """EST = lead + A + M + B, the factorization (A + the first k bytes of M laid over the intron, the rest of M laid in
    front of B + B): the search between the two finds M"""
    k = int(rng.integers(0, L.m_len + 1)) if k is None else k
    est = lead + L.seq(L.a, L.a_len) + L.seq(L.m, L.m_len) + L.seq(L.b, L.b_len)
    e0 = len(lead)
    x1 = (e0, e0 + L.a_len + k - 1, L.a, L.a + L.a_len + k - 1)
    x2 = (e0 + L.a_len + k, len(est) - 1, L.b - (L.m_len - k), L.b + L.b_len - 1)
    return est, [x1, x2]


def build_prefix_cases(w, reps):
    rng = w.rng
    for rep in range(reps):
        L = w.locus()
        w.add("prefix_found", *prefix_case(L))
        # EST_start 6 and 7: a small exon of 6 / 7 bytes in front
        for n in (6, 7):
            L = w.locus(s_len=n)
            w.add("est_start_%d" % n, *prefix_case(L))
        # the gate e1len + EST_start at 28 and 29: a short first exon
        for total in (28, 29):
            L = w.locus(s_len=10, a_len=total - 10)
            w.add("gate_%d" % total, *prefix_case(L))
        # two longest factors of equal length: S planted twice in front of the exon, and a piece that holds S twice
        L = w.locus(s_len=10)
        L.g[L.s - 40:L.s - 30] = L.seq(L.s, 10)
        w.add("tie_gen", *prefix_case(L))
        L = w.locus(s_len=9)
        s9 = L.seq(L.s, 9)
        w.add("tie_est", *prefix_case(L, flank=s9 + b"C" if s9[-1:] != b"C" else s9 + b"G"))
        # EST_start 46 and 47 (pe turns from right to misused), and beyond: a flank of unrelated bytes in front of S
        for start in (46, 47, 60, 120):
            L = w.locus(s_len=12)
            w.add("est_start_%d" % start, *prefix_case(L, flank=RL.rnd(rng, start - 12)))
        # the exon's first bytes differ from the sequence: the edit distance runs
        L = w.locus()
        est, ex = prefix_case(L)
        est = bytearray(est)
        est[ex[0][0] + 4] = other_base(est[ex[0][0] + 4])
        w.add("prefix_ed", est, ex)
        # a refinement that is refused: S matches for six bytes only and the rest is noise
        L = w.locus(s_len=16)
        piece = bytearray(RL.rnd(rng, 16))
        piece[0:7] = L.seq(L.s, 7)
        w.add("borders_no", *prefix_case(L, s_keep=bytes(piece)))
        # an intron one base short of min_intron_length, and one that fits; min_intron_length <= 0
        L = w.locus()
        est, ex = prefix_case(L)
        w.add("intron_short", est, ex, mil=L.i[0] + 1)
        w.add("intron_fits", est, ex, mil=L.i[0])
        w.add("mil_zero", est, ex, mil=0)
        w.add("mil_negative", est, ex, mil=-5)
        # a non-canonical pair: GC .. AG
        L = w.locus()
        L.g[L.s + L.s_len:L.s + L.s_len + 2] = b"GC"
        w.add("site_GC", *prefix_case(L))
        # off_p - pe below 6: a small exon of which only a part in front of the cut matches (the cut at 6 is the first
        # allowed), and wrapping: EST_start beyond 46 with the factor late in the piece
        L = w.locus(s_len=8)
        est, ex = prefix_case(L, cut=3)
        w.add("offp_short", est, ex)
        # ... a small exon of eight bytes behind four unrelated ones: pe = 4, the cut at 8
        for n_junk in (3, 4):
            L = w.locus(s_len=8)
            w.add("offp_below_6", *prefix_case(L, flank=RL.rnd(rng, n_junk)))
        # allelen at the cap and one beyond: EST_start + 23 - pe with the factor at the piece's first byte
        for allelen in (256, 257, 256, 257):
            start = allelen - 23 + 0
            L = w.locus(s_len=12)
            flank = RL.rnd(rng, start - 46) + L.seq(L.s, 12) + RL.rnd(rng, 22)
            w.add("window_%d" % allelen, *prefix_case(L, flank=flank))
        # one N in the piece, two Ns
        for n_wild in (1, 2):
            L = w.locus(s_len=14)
            piece = bytearray(L.seq(L.s, 14))
            piece[5] = ord("N")
            if n_wild == 2:
                piece[9] = ord("n")
            w.add("piece_%dn" % n_wild, *prefix_case(L, s_keep=bytes(piece)))
        # a lower-case byte in the piece (refused = 3 too)
        L = w.locus(s_len=14)
        piece = bytearray(L.seq(L.s, 14))
        piece[4] = piece[4] | 32
        w.add("piece_lower", *prefix_case(L, s_keep=bytes(piece)))


def build_between_cases(w, reps):
    rng = w.rng
    for rep in range(reps):
        L = w.locus()
        for k in (0, L.m_len // 2, L.m_len):
            w.add("between_found_k%d" % k, *between_case(L, k=k))
        # the gate e1len + e2len at 51 and 52
        for total in (51, 52):
            L = w.locus(a_len=20, b_len=total - 20 - 10, m_len=10)
            w.add("pair_gate_%d" % total, *between_case(L, k=5))
        # e1slen bound by the genomic length: the first exon has fewer genomic bytes than EST bytes
        L = w.locus()
        est, ex = between_case(L, k=4)
        ex[0] = (ex[0][0], ex[0][1], ex[0][3] - 14, ex[0][3])
        w.add("e1slen_by_gen", est, ex)
        # sed + ped 2 and 3 over a classified intron: A and B exact but for 2 / 3 substituted bytes near the junction, no M
        for n_err in (0, 2, 3):
            L = w.locus()
            est = bytearray(L.seq(L.a, L.a_len) + L.seq(L.b, L.b_len))
            for j in range(n_err):
                p = L.a_len - 3 - 4 * j if j != 1 else L.a_len + 4
                est[p] = other_base(est[p])
            w.add("dist_%d" % n_err, est, [(0, L.a_len - 1, L.a, L.a + L.a_len - 1), (L.a_len, len(est) - 1, L.b, L.b + L.b_len - 1)])
        # class 2 with sed + ped = 0: exact exons around an intron without its GT
        L = w.locus()
        L.g[L.a + L.a_len:L.a + L.a_len + 2] = b"CC"
        est = L.seq(L.a, L.a_len) + L.seq(L.b, L.b_len)
        w.add("class2_dist_0", est, [(0, L.a_len - 1, L.a, L.a + L.a_len - 1), (L.a_len, len(est) - 1, L.b, L.b + L.b_len - 1)])
        # an N inside efact
        L = w.locus()
        est, ex = between_case(L, k=3)
        est = bytearray(est)
        est[L.a_len + L.m_len // 2] = ord("N")
        w.add("efact_n", est, ex)
        # a small exon of six bytes
        L = w.locus(m_len=6)
        w.add("winner_6", *between_case(L, k=3))
        # the small exon planted twice inside the intron window: a tie between candidates
        L = w.locus(m_len=9, intr=(150, 160))
        L.g[L.b - 80:L.b - 71] = L.seq(L.m, 9)
        L.g[L.b - 71:L.b - 69] = b"GT"
        L.g[L.b - 82:L.b - 80] = b"AG"
        w.add("search_tie", *between_case(L, k=4))
        # no candidate: the bytes between A and B occur nowhere in the intron
        L = w.locus()
        est = L.seq(L.a, L.a_len) + RL.rnd(rng, 11) + L.seq(L.b, L.b_len)
        w.add("search_none", est, [(0, L.a_len + 4, L.a, L.a + L.a_len + 4), (L.a_len + 5, len(est) - 1, L.b - 6, L.b + L.b_len - 1)])
        # short borders: f1slen / f2plen below 6 (noise at the exon ends), no room on the sequence, no room on the EST
        L = w.locus()
        est, ex = between_case(L, k=5)
        e = bytearray(est)
        for j in range(1, 23, 4):
            e[L.a_len - j] = other_base(e[L.a_len - j])
        w.add("gate_f1", e, ex)
        e = bytearray(est)
        for j in range(0, 23, 4):
            e[L.a_len + L.m_len + j] = other_base(e[L.a_len + L.m_len + j])
        w.add("gate_f2", e, ex)
        w.add("gate_room", est, ex, mil=200)
        # the extension loop: an exact first exon, and a second one whose first three EST bytes are wrong, the first of them
        # being the sequence's second
        for _ in range(2):
            L = w.locus()
            e = bytearray(L.seq(L.a, L.a_len) + L.seq(L.b, L.b_len))
            e[L.a_len] = L.g[L.b + 1]
            e[L.a_len + 1] = other_base(L.g[L.b + 1])
            e[L.a_len + 2] = other_base(L.g[L.b + 2])
            w.add("extension", e, [(0, L.a_len - 1, L.a, L.a + L.a_len - 1), (L.a_len, len(e) - 1, L.b, L.b + L.b_len - 1)])
        # no room on the EST: a first exon of eight bytes, and a second one that agrees with the sequence for seven
        L = w.locus(a_len=8, b_len=50)
        e = bytearray(L.seq(L.a, 8) + L.seq(L.b, 50))
        for j in range(8 + 7, 8 + 23, 2):
            e[j] = other_base(e[j])
        w.add("gate_elen", e, [(0, 7, L.a, L.a + 7), (8, 57, L.b, L.b + 49)])
    # insertions at three introns of one list, 64 exons that grow, 65 exons
    for rep in range(reps):
        Ls = [w.locus() for _ in range(3)]
        est, exons = b"", []
        for L in Ls:
            e, x = between_case(L, k=L.m_len // 2, lead=est)
            est, exons = e, exons + x
        w.add("three_insertions", est, exons)
        for n in (64, 65):
            L = w.locus()
            e0, x0 = between_case(L, k=4)
            est, exons = bytearray(e0), list(x0)
            at = L.end + 40
            # further exons of 3 bytes each, 9 apart, copied from what follows the locus
            G = w.g
            while len(exons) < n:
                exons.append((len(est), len(est) + 2, at, at + 2))
                est += G[at:at + 3]
                at += 9
            assert at < len(G)
            w.add("exons_%d" % n, est, exons)


def build_clean_cases(w, reps):
    rng = w.rng
    for rep in range(reps):
        # a noisy middle exon with best-run ties: three exons, the middle one scrambled, both sides cover equally
        L = w.locus(a_len=50, b_len=50, m_len=16)
        est = bytearray(L.seq(L.a, 50) + L.seq(L.m, 16) + L.seq(L.b, 50))
        for j in range(50, 66, 2):
            est[j] = other_base(est[j])
        w.add("noisy_middle_tie", est, [(0, 49, L.a, L.a + 49), (50, 65, L.m, L.m + 15), (66, 115, L.b, L.b + 49)])
        # end exons of 9, 10, 19 and 20 genomic bytes; with both sites, without the donor, without the acceptor, differing
        for n in (9, 10, 19, 20):
            for kind in ("ok", "no_donor", "no_acceptor", "differs"):
                for end in (0, 1):
                    L = w.locus(a_len=60, b_len=60, z_len=n, s_len=n)
                    if end == 0:        # [S'] i1 [A]: the head S' of n bytes
                        est = bytearray(L.seq(L.s, n) + L.seq(L.a, 60))
                        ex = [(0, n - 1, L.s, L.s + n - 1), (n, n + 59, L.a, L.a + 59)]
                        d, a, mine = L.s + n, L.a, 2
                    else:               # [B] i4 [Z]: the tail Z of n bytes
                        est = bytearray(L.seq(L.b, 60) + L.seq(L.z, n))
                        ex = [(0, 59, L.b, L.b + 59), (60, 59 + n, L.z, L.z + n - 1)]
                        d, a, mine = L.b + 60, L.z, 62
                    if kind == "no_donor":
                        L.g[d + 1:d + 2] = b"A"
                    if kind == "no_acceptor":
                        L.g[a - 2:a - 1] = b"C"
                    if kind == "differs":
                        est[mine] = other_base(est[mine])
                    w.add("end_%d_%s_%d" % (n, kind, end), est, ex)
        # a list emptied at each verdict: every exon noisy; one short exon alone
        L = w.locus()
        est = bytearray(L.seq(L.a, L.a_len))
        for j in range(0, L.a_len, 3):
            est[j] = other_base(est[j])
        w.add("emptied_noisy", est, [(0, L.a_len - 1, L.a, L.a + L.a_len - 1)])
        L = w.locus(s_len=9)
        w.add("emptied_external", L.seq(L.s, 9), [(0, 8, L.s, L.s + 8)])
        # an answer that differs between the working and the original sequence: the working one has its first exon masked
        L = w.locus()
        orig = L.seq(L.a, L.a_len) + L.seq(L.b, L.b_len)
        work = b"#" * 30 + orig[30:]
        ex = [(0, L.a_len - 1, L.a, L.a + L.a_len - 1), (L.a_len, len(orig) - 1, L.b, L.b + L.b_len - 1)]
        w.add("orig_decides", work, ex, orig=orig)
        # an exon inserted by step 2 that step 3 drops: the original sequence differs inside M
        L = w.locus(m_len=14)
        est, ex = between_case(L, k=6)
        orig = bytearray(est)
        for j in range(L.a_len, L.a_len + 14, 3):
            orig[j] = other_base(orig[j])
        w.add("inserted_dropped", est, ex, orig=bytes(orig))
        # a disordered list
        L = w.locus()
        est, ex = between_case(L, k=3)
        w.add("disordered_pair", est, [ex[0], (ex[1][0], ex[1][1], ex[0][3], ex[1][3])])
        w.add("disordered_exon", est, [(ex[0][1], ex[0][0], ex[0][2], ex[0][3]), ex[1]])
    # K-band bounds 31 and 32: a genomic exon length of 1 033 and 1 034 (over several loci's worth of sequence)
    for n in (1033, 1034) * reps:
        L = w.locus()
        w.locus()
        est = w.g[L.s:L.s + n]
        w.add("kband_%d" % (31 if n == 1033 else 32), bytes(est), [(0, n - 1, L.s, L.s + n - 1)])


def mini_world(seed, kind):
    """a sequence of one locus with one case of `kind` between two ordinary neighbours (a small exon between two exons, and
    two exact exons: both begin at the EST's first byte and ask nothing of the prefix), for what depends on the whole
    sequence in front of the first exon: the first byte that is no upper-case ACGT where the exon begins (`first_bad_at`)
    or one byte earlier (`first_bad_past`); splice sites in mixed and lower case in front of the exon (`site_*`: refused = 3)
    and AT its start -- the exon laid over a short intron and the true exon behind it, so that GEN_start is the first such
    byte and the query is answered (`gtag_lower`, `gtag_mixed`); a piece that shares five / six bytes with the little there
    is in front (`cflen_*`)"""
    w = World(seed, 1)
    rng = w.rng
    mil = 60
    if kind in ("first_bad_at", "first_bad_past"):
        L = w.locus()
        shift = 0 if kind == "first_bad_at" else 1
        w.g[L.a - shift] = w.g[L.a - shift] | 32
        est, ex = prefix_case(L)
        est = bytearray(est)
        est[ex[0][0]] = w.g[L.a]                             # (the exon's first byte on the EST follows the sequence)
    elif kind in ("site_mixed", "site_lower"):
        L = w.locus()
        d, a = L.s + L.s_len, L.a
        if kind == "site_mixed":
            L.g[d:d + 2] = b"gT"
        else:
            L.g[d:d + 2], L.g[a - 2:a] = b"gt", b"ag"
        est, ex = prefix_case(L)
    elif kind in ("gtag_lower", "gtag_mixed"):               # [S] gt..ag [A]: S, then an intron of 4 to 10 bytes, then A
        k = int(rng.integers(4, 11))
        L = w.locus(s_len=14)
        gs = L.s + 14
        L.a = gs + k
        w.g[gs:gs + k] = b"gt" + RL.rnd(rng, k - 4).lower() + (b"ag" if kind == "gtag_lower" else b"aG")
        w.g[L.a:L.a + L.a_len] = RL.rnd(rng, L.a_len)
        w.g[L.a + L.a_len:L.a + L.a_len + 2] = b"GT"
        est = L.seq(L.s, 14) + L.seq(L.a, 15)
        ex = [(14, 28, gs, gs + k + 14)]
        mil = (0, 4)[int(rng.integers(2))]
    else:                                                    # cflen_5, cflen_6: the locus at the sequence's first bytes
        n = int(kind[-1])
        w.g[:] = w.g[:LOCUS]
        L = Locus(w.g, 0, rng, s_len=12, pad=2, intr=(40, 50))
        piece = bytearray(RL.rnd(rng, 12))
        piece[3:3 + n] = L.seq(L.s + 3, n)
        for j in (2, 3 + n):
            piece[j] = other_base(L.g[L.s + j])
        est, ex = prefix_case(L, s_keep=bytes(piece))
        mil = 30
    w.add("beside_between", *between_case(L, k=L.m_len // 2), mil=mil)
    w.add(kind, est, ex, mil=mil)
    plain = L.seq(L.a, L.a_len) + L.seq(L.b, L.b_len)
    w.add("beside_plain", plain, [(0, L.a_len - 1, L.a, L.a + L.a_len - 1), (L.a_len, len(plain) - 1, L.b, L.b + L.b_len - 1)], mil=mil)
    return bytes(w.g), w.cases


MINI_KINDS = ("first_bad_at", "first_bad_past", "site_mixed", "site_lower", "gtag_lower", "gtag_mixed", "cflen_5", "cflen_6")


def make_worlds(seed, reps=MIN_PER_TAG):
    """[(seed, the sequence, [(name, orig, est, exons, min_intron_length)])]: the hand-made cases of every builder over one
    sequence, then the one-locus sequences of mini_world"""
    w = World(seed, reps * 170 + 40)
    build_prefix_cases(w, reps)
    build_between_cases(w, reps)
    build_clean_cases(w, reps)
    w.g[200 + w.used * LOCUS:] = b""
    out = [(seed, bytes(w.g), w.cases)]
    for k, kind in enumerate(MINI_KINDS):
        for rep in range(2 * reps):
            s2 = seed + 1000 * (k + 1) + rep
            g, cases = mini_world(s2, kind)
            out.append((s2, g, cases))
    return out


def generated(seed, n, n_loci=120):
    """(the sequence, n fresh ordinary factorizations over its loci): prefix small exons, small exons between two exons
    laid over the introns, short or noisy end exons, and plain factorizations with nothing to do; every one is PGPU_OK"""
    w = World(seed, n_loci)
    loci = [w.locus() for _ in range(n_loci)]
    g = bytes(w.g)
    rng = np.random.default_rng(seed + 1)
    out = []
    for _ in range(n):
        L = loci[int(rng.integers(n_loci))]
        r = rng.random()
        mil = int((4, 40, 60, 60)[int(rng.integers(4))])
        if r < 0.25:                                         # S in front of A (+ B): step 1
            flank = RL.rnd(rng, int(rng.integers(0, 25))) if rng.random() < 0.5 else b""
            est, ex = prefix_case(L, flank=flank)
            if rng.random() < 0.5:
                ex.append((len(est), len(est) + L.b_len - 1, L.b, L.b + L.b_len - 1))
                est += g[L.m - 0:L.m] + g[L.b:L.b + L.b_len]
            orig = est
        elif r < 0.55:                                       # M between A and B: step 2
            est, ex = between_case(L, rng=rng, lead=RL.rnd(rng, int(rng.integers(0, 6))))
            orig = est
        elif r < 0.80:                                       # step 3 has something to drop
            est = g[L.a:L.a + L.a_len] + g[L.b:L.b + L.b_len]
            ex = [(0, L.a_len - 1, L.a, L.a + L.a_len - 1), (L.a_len, len(est) - 1, L.b, L.b + L.b_len - 1)]
            orig = est
            if rng.random() < 0.5:                           # a short last exon
                n_z = int(rng.integers(4, 10))
                ex.append((len(est), len(est) + n_z - 1, L.z, L.z + n_z - 1))
                est = orig = est + g[L.z:L.z + n_z]
            else:                                            # the original sequence is noisy over the first exon
                o = bytearray(est)
                for j in range(2, L.a_len, 4):
                    o[j] = other_base(o[j])
                orig = bytes(o)
        else:                                                # nothing to do, now and then a substituted base
            parts = [(L.a, L.a_len), (L.b, L.b_len), (L.z, L.z_len)][:int(rng.integers(1, 4))]
            est, ex = bytearray(), []
            for at, ln in parts:
                ex.append((len(est), len(est) + ln - 1, at, at + ln - 1))
                est += g[at:at + ln]
            if rng.random() < 0.4:
                p = int(rng.integers(len(est)))
                est[p] = other_base(est[p])
            est = orig = bytes(est)
        out.append(("generated", bytes(orig), bytes(est), [tuple(e) for e in ex], mil))
    return g, out


# ---- the arrays of the entry ------------------------------------------------------------------------------------------
def batch_arrays(cases):
    """cases of (name, orig, est, exons, ...) -> (ests, exons array, queries array) in the layouts of the entry"""
    return TL.batch_arrays([c[:4] for c in cases])


def expect_arrays(exons, queries, answers):
    """answers of small() per query -> the three arrays of the entry: 2 * len(exons) slots, a query's list at 2 * first_exon"""
    from pintron_amd import capi
    out_exons = np.zeros(2 * len(exons), dtype=np.dtype(capi.FACTOR_DTYPE))
    out_steps = np.zeros(2 * len(exons), dtype=np.uint8)
    res = np.zeros(len(answers), dtype=np.dtype(capi.SMALL_RESULT_DTYPE))
    for i, a in enumerate(answers):
        status, refused, verdict, prefix_added, n_added, n_list, first, kept, lst, steps = a
        res[i] = (status, refused, verdict, prefix_added, 0, n_added, n_list, first, kept)
        at = 2 * int(queries[i]["first_exon"])
        assert len(lst) <= 2 * int(queries[i]["n_exons"])
        for k, (e, s) in enumerate(zip(lst, steps)):
            out_exons[at + k] = tuple(e)
            out_steps[at + k] = s
    return out_exons, out_steps, res


def _case_dicts(rows):
    cases = []
    for name, orig, est, ex, mil, res, after, steps, tags, witnesses in rows:
        est = est.encode()
        cases.append(dict(name=name, orig=est if orig is None else orig.encode(), est=est, exons=[tuple(e) for e in ex], mil=mil,
                          answer=tuple(res) + ([tuple(e) for e in after], list(steps)), tags=set(tags), witnesses=witnesses))
    return cases


_fixture = []


def load_fixture():
    """([(genomic bytes, [case dicts: name, orig, est, exons, mil, answer (the tuple of small()), tags, witnesses])], {source:
    [case dicts]}): the hand-made cases over their seeded sequences, and the ones of the real inputs (over their own)"""
    if not _fixture:
        doc = json.load(gzip.open(FIXTURE, "rt"))
        worlds = []
        for wd in doc["worlds"]:
            g = bytearray(RL.rnd(np.random.default_rng(wd["seed"]), wd["length"]))
            for pos, s in wd["edits"]:
                g[pos:pos + len(s)] = s.encode()
            worlds.append((bytes(g), _case_dicts(wd["cases"])))
        _fixture.append((worlds, {src: _case_dicts(rows) for src, rows in doc["real"].items()}))
    return _fixture[0]


def quints(cases):
    return [(c["name"], c["orig"], c["est"], c["exons"], c["mil"]) for c in cases]


# ---- today's device route ---------------------------------------------------------------------------------------------
class _Asked(Exception):
    pass


class _DeviceOps:
    """answers from the rounds run so far; a question without one is noted, and the query that asked waits for the next round"""

    def __init__(self, gen):
        self.gen = gen
        self.first_bad = first_bad(gen)
        self.got, self.want = {}, {}

    def _ask(self, key):
        if key in self.got:
            return self.got[key]
        self.want.setdefault(key, len(self.want))
        raise _Asked()

    def lcf_prefix(self, gstart, piece):
        r = self._ask(("lcfp", gstart, piece))
        return r["len"], r["occ1"], r["occ2"]

    def ed(self, a, b):
        return self._ask(("ed", a, b))["score"]

    def borders(self, p, gstart, glen, p0, p1, max_errs):
        return self._ask(("borders", p, gstart, glen, p0, p1, max_errs))

    def lcf(self, a, b):
        r = self._ask(("lcf", a, b))
        return r["len"], r["occ1"], r["occ2"]

    def classify(self, start, end):
        return self._ask(("class", start, end))

    def sexon(self, efact, allgstart, allglen, f1slen, f2plen, mil, info=None):
        return self._ask(("sexon", efact, allgstart, allglen, f1slen, f2plen, mil))

    def kband(self, g, e, ub):
        return bool(self._ask(("kband", g, e, ub))["ok"])


def device_route(ctx, idx, gen: bytes, cases, clock=None):
    """cases of (name, orig, est, exons, mil) -> the answers of small(), every question asked of the device: the dynamic
    programs as jobs of one DP plan per round (the prefix's common factor with PGPU_JOB_A_GENOMIC, its refinement with
    PGPU_JOB_B_GENOMIC), the intron classes through pgpu_index_classify and the searches through pgpu_index_small_exons, with
    the glue of small() on the host.  `clock` (a dict) receives "library_s", the seconds inside the library's entry points,
    "jobs" and "rounds"."""
    import time
    from pintron_amd import capi
    ops = _DeviceOps(gen)
    inside, n_jobs, rounds = 0.0, 0, 0
    answers = [None] * len(cases)
    kinds = {"lcfp": capi.LCF, "lcf": capi.LCF, "ed": capi.ED, "borders": capi.BORDERS, "kband": capi.KBAND}
    while True:
        for k, (_, orig, est, ex, mil) in enumerate(cases):
            if answers[k] is None:
                try:
                    answers[k] = small(orig, est, gen, ex, mil, ops=ops)
                except _Asked:
                    pass
        if not ops.want:
            break
        keys = sorted(ops.want, key=ops.want.get)
        dp = [k for k in keys if k[0] in kinds]
        if dp:
            jl = capi.JobList()
            for key in dp:
                if key[0] == "lcfp":
                    jl.add(capi.LCF, bytes(key[1]), key[2], a_gen_off=0)
                elif key[0] in ("lcf", "ed"):
                    jl.add(kinds[key[0]], key[1], key[2])
                elif key[0] == "kband":
                    jl.add(capi.KBAND, key[1], key[2], p0=key[3])
                else:
                    _, p, gstart, glen, p0, p1, max_errs = key
                    jl.add(capi.BORDERS, p, bytes(glen), p0=p0, p1=p1, p2=max_errs, b_gen_off=gstart,
                           tail=min(2, len(gen) - (gstart + glen)))
            t0 = time.perf_counter()
            got = capi.run_jobs(ctx, jl, idx)
            inside += time.perf_counter() - t0
            for key, o in zip(dp, got):
                assert o["status"] == 0, (key[0], o)
                ops.got[key] = o
            n_jobs += len(dp)
        cl = [k for k in keys if k[0] == "class"]
        if cl:
            t0 = time.perf_counter()
            got = idx.classify([k[1] for k in cl], [k[2] for k in cl])
            inside += time.perf_counter() - t0
            for key, o in zip(cl, got):
                ops.got[key] = int(o)
            n_jobs += len(cl)
        sx = [k for k in keys if k[0] == "sexon"]
        if sx:
            blob, rows, off = [], [], 0
            for _, efact, allgstart, allglen, f1, f2, mil in sx:
                rows.append((off, len(efact), allgstart, allglen, f1, f2, mil))
                blob.append(efact)
                off += len(efact)
            t0 = time.perf_counter()
            got = idx.small_exons(b"".join(blob), rows)
            inside += time.perf_counter() - t0
            for key, o in zip(sx, got):
                assert int(o["status"]) == 0
                ops.got[key] = (int(o["len"]), int(o["offstart"]), int(o["offend"]), int(o["gpos"]))
            n_jobs += len(sx)
        ops.want = {}
        rounds += 1
    if clock is not None:
        clock["library_s"], clock["jobs"], clock["rounds"] = inside, n_jobs, rounds
    return answers


# ---- the host's own routines: ef_chain_small, the oracle as backend ---------------------------------------------------
class Host(TL.Host):
    def __init__(self, genomic: bytes):
        import ctypes as C
        TL.Host.__init__(self, genomic)
        H = self.H
        H.ef_seq_index_kmers.argtypes = [C.c_void_p]
        H.ef_classify_prepare.argtypes = [C.c_void_p]
        H.ef_chain_small.restype = C.c_uint
        H.ef_chain_small.argtypes = [C.c_char_p, C.c_char_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint, C.c_uint,
                                     C.POINTER(C.c_uint)]
        H.ef_seq_index_kmers(self.seq)
        H.ef_classify_prepare(self.seq)
        H.ef_config_set_min_intron_length.argtypes = [C.c_void_p, C.c_int]

    def small(self, orig: bytes, est: bytes, exons, mil: int):
        """ef_chain_small -> (1 when the cleaning emptied the list, the exons left)"""
        import ctypes as C
        self._set_mil(mil)
        n = len(exons)
        cap = 2 * n
        ex = (C.c_int32 * (4 * cap))(*[v for e in exons for v in e])
        n_out = C.c_uint(0)
        emptied = self.H.ef_chain_small(est, orig, self.seq, self.cfg, self.be, ex, n, cap, C.byref(n_out))
        assert n_out.value <= cap
        return emptied, [tuple(ex[4 * k:4 * k + 4]) for k in range(n_out.value)]

    def _set_mil(self, mil):
        self.H.ef_config_set_min_intron_length(self.cfg, mil)


def agrees_with_host(answer, host_answer):
    """what ef_chain_small can say of one accepted query, against the restatement's answer"""
    assert answer[0] == OK
    return host_answer == (1 if answer[2] else 0, kept_exons(answer) if answer[2] == 0 else [])
