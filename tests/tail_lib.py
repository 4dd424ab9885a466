"""CPU restatement of pgpu_index_tail_chains: what est-fact does to one factorization directly behind the refinement loop --
correct_composition_tail and detect_polyA_signal (src/detect-polya.c:42-166), then remove_invalid_factorizations,
recover_lost_prefixes_and_suffixes and remove_false_small_exons (src/factorization-refinement.c:120-165, :959-1266).

tail            the five steps in Python, lists and loops as the reference writes them, over an `ops` object that answers
                the three device questions (longest affix, edit distance, border refinement): OracleOps asks
                tests/oracle_lib.py; the caps of the entry.
einval          the PGPU_EINVAL rules of the entry for one call.
make_world      hand-made cases over a seeded sequence of GEN_LEN bases, one builder per tag of the fixture's cover; a
                builder that writes into the sequence does so inside a slot of its own in front of READ_ZONE.
generated       fresh ordinary factorizations over a world's sequence, read only (the GPU test's 2 000).
batch_arrays / expect_arrays   the arrays of the entry for a batch and for its answers.
device_route    today's route on the device: the same questions as PGPU_DP_AFFIX, PGPU_DP_ED and PGPU_DP_BORDERS jobs of
                DP plans (a question may need an earlier answer: one plan per round), the glue of tail() on the host.
load_fixture    tests/golden/tail_chains.json.gz (tools/make_tail_golden.py).
"""
import gzip
import json
import os

import numpy as np

import cand_lib as KL
import oracle_lib as O
import refine_lib as RL

FIXTURE = os.path.join(RL.ROOT, "tests", "golden", "tail_chains.json.gz")
OK, ERANGE, EINVAL = 0, -34, -22
MAX_EXONS = 64            # PGPU_TAIL_MAX_EXONS
MAX_AFFIX = 256           # PGPU_TAIL_MAX_AFFIX
MAX_SMALL_WINDOW = 128    # PGPU_TAIL_MAX_SMALL_WINDOW
MAX_SMALL_GEN = 256       # PGPU_TAIL_MAX_SMALL_GEN
UB_MED_EXON = 100         # _UB_MED_EXON_
AFFIXES_LENGTH = 5        # _AFFIXES_LENGTH_
MAX_ERROR_RATE = 0.17     # _MAX_ERROR_RATE_
NOT_ANALYSED, REFUSED, BURSET_FELL, REMOVED = 0, 1, 2, 3
STEP_PREFIX, STEP_SUFFIX, STEP_TAIL = 0x10, 0x20, 0x40

# the cover of the fixture (tools/make_tail_golden.py asks for MIN_PER_TAG cases of each)
TAGS = ("ext_0", "ext_63", "ext_64", "ext_65", "ext_to_est_end", "ext_to_gen_end",
        "polyA_yes", "polyA_eight", "hex_AATAAA", "hex_ATTAAA", "hex_aataaa", "hex_attaaa", "hex_mixed_case", "hex_cut",
        "cancel_run6", "cancel_count7",
        "inv_est_exon", "inv_gen_exon", "inv_est_pair", "inv_gen_pair",
        "pre_recovered", "pre_skipped", "pre_no_cut", "pre_tie", "suf_recovered", "suf_skipped", "suf_no_cut", "suf_tie",
        "affix_64", "affix_65", "affix_256", "affix_257",
        "removed", "removed_twice", "removed_at_1", "refine_refused", "burset_lower", "burset_equal",
        "exon_100", "exon_101", "window_128", "window_129", "gen_256", "gen_257",
        "front_suffix", "exons_64", "exons_65", "orig_differs")
MIN_PER_TAG = 10
REPS = 16                 # cases a builder makes of each kind: an aim only steers, the tag is what tail() measures
REFUSED_TAGS = ("affix_257", "window_129", "gen_257", "exons_65")
_HEXAMERS = (b"aataaa", b"AATAAA", b"attaaa", b"ATTAAA")


class OracleOps:
    """the three questions, answered by the CPU oracle"""

    def affix(self, e: bytes, g: bytes):
        return O.longest_affix(e, g)

    def ed(self, a: bytes, b: bytes):
        return O.edit_distance(a, b)

    def borders(self, p: bytes, gen: bytes, gstart: int, gend: int, max_errs: int):
        return O.refine_borders(p, gen[gstart:gend], 0, len(p), max_errs, gen[gend:gend + 2])


ORACLE = OracleOps()


class _Refuse(Exception):
    pass


def _is_a(c):
    return c in (97, 65)


def correct_tail(orig: bytes, gen: bytes, tail):
    """correct_composition_tail (src/detect-polya.c:42-71): the tail exon's two ends moved; returns the bases added"""
    i, j = tail[1] + 1, tail[3] + 1
    while i < len(orig) and j < len(gen) and gen[j] == orig[i]:
        i += 1
        j += 1
    added = i - (tail[1] + 1)
    tail[1], tail[3] = i - 1, j - 1
    return added


def detect_polyA(orig: bytes, gen: bytes, tail, info):
    """detect_polyA_signal (:73-166), the loops as written -> (polyA, polyadenil)"""
    el, gl = len(orig), len(gen)
    est_end, gen_end = tail[1], tail[3]
    cl = orig[est_end + 1:]
    cll = el - est_end - 1 if est_end + 1 <= el else 0
    i = matches = 0
    stop = False
    while i < cll and not stop:
        if _is_a(cl[i]):
            if matches >= 8:
                stop = True
            else:
                matches += 1
                i += 1
        else:
            if matches >= 8:
                stop = True
            else:
                i = cll
    if not stop and cll == 8 and matches == 8:
        info["polyA_eight"] = True
    polyadenil = False
    if stop:
        i = gen_end - 39 if gen_end - 39 > 0 else 0
        while i <= gen_end and not polyadenil:
            if _is_a(gen[i]):
                pas = gen[i:i + 6]                           # real_substring(i, 6, gen): stops at the terminator
                if pas in _HEXAMERS:
                    polyadenil = True
                    info["hex_" + pas.decode()] = True
                elif len(pas) < 6 and any(h.startswith(pas) for h in _HEXAMERS):
                    info["hex_cut"] = True
                elif pas.upper() == b"AATAAA" or pas.upper() == b"ATTAAA":
                    info["hex_mixed_case"] = True
            i += 1
        if polyadenil:
            info.pop("hex_cut", None)
            info.pop("hex_mixed_case", None)
        i = gen_end - 9 if gen_end - 9 > 0 else 0
        matches = 0
        while i <= gen_end + 10 and stop and i < gl:
            if matches >= 6:
                stop = False
                info["cancel_run6"] = True
            else:
                if _is_a(gen[i]):
                    matches += 1
                else:
                    matches = 0
                i += 1
        if stop:
            i = gen_end + 1
            count = 0
            while i <= gen_end + 10 and stop and i < gl:
                if count >= 7:
                    stop = False
                    info["cancel_count7"] = True
                else:
                    if _is_a(gen[i]):
                        count += 1
                    i += 1
        if stop:
            info["polyA_yes"] = True
    return stop, polyadenil


def invalid(ex, info):
    """remove_invalid_factorizations (:121-165) on one factorization"""
    inv = False
    prev = None
    for x in ex:
        if x[0] > x[1]:
            info["inv_est_exon"] = inv = True
        elif x[2] > x[3]:
            info["inv_gen_exon"] = inv = True
        elif prev is not None and prev[1] >= x[0]:
            info["inv_est_pair"] = inv = True
        elif prev is not None and prev[3] >= x[2]:
            info["inv_gen_pair"] = inv = True
        if inv:
            break
        prev = x
    return inv


def _affix_tie(e: bytes, g: bytes):
    """whether more than one cell of find_longest_affix's scan has the best weight (small windows only: the tag's cost)"""
    if len(e) * len(g) > 4000:
        return False
    prev = list(range(len(g) + 1))
    best, n_best = None, 0
    for i in range(1, len(e) + 1):
        cur = [i] + [0] * len(g)
        for j in range(1, len(g) + 1):
            cur[j] = min(prev[j - 1] + (e[i - 1] != g[j - 1]), prev[j] + 1, cur[j - 1] + 1)
            if e[i - 1] == g[j - 1] and 200 * cur[j] <= 17 * (i + j):
                w = (cur[j], i + j)                          # weight v / (e + g), compared by cross-multiplication
                if best is None or w[0] * best[1] < best[0] * w[1]:
                    best, n_best = w, 1
                elif w[0] * best[1] == best[0] * w[1]:
                    n_best += 1
        prev = cur
    return n_best > 1


def recover_affixes(est: bytes, gen: bytes, ex, steps, ops, info):
    """recover_lost_prefixes_and_suffixes (:1177-1266) on one factorization -> the `recovered` bits"""
    tote, totg = len(est), len(gen)
    ff, fl = ex[0], ex[-1]
    pre = suf = None
    if ff[0] > 0 and ff[2] > 0:
        flen = min(ff[0], ff[2])
        cap = int((1.0 + MAX_ERROR_RATE) * flen)
        elen, glen = min(ff[0], cap), min(ff[2], cap)
        if est[ff[0] - 1] != gen[ff[2] - 1]:
            if elen > MAX_AFFIX and not info.get("no_caps"):
                info["affix_257"] = info.get("affix_257") or elen == MAX_AFFIX + 1
                raise _Refuse("a lost prefix window of %d EST bytes" % elen)
            pre = (est[ff[0] - elen:ff[0]][::-1], gen[ff[2] - glen:ff[2]][::-1])
        else:
            info["pre_skipped"] = True
    if tote - fl[1] > 1 and totg - fl[3] > 1:
        flen = min(tote - fl[1] - 1, totg - fl[3] - 1)
        elen = min(tote - fl[1] - 1, int(1.0 + MAX_ERROR_RATE) * flen)           # the cast binds first: 1 * flen
        glen = min(totg - fl[3] - 1, int(1.0 + MAX_ERROR_RATE) * flen)
        if est[fl[1]] != gen[fl[3]]:                                             # the windows start ON the last byte
            if elen > MAX_AFFIX and not info.get("no_caps"):
                info["affix_257"] = info.get("affix_257") or elen == MAX_AFFIX + 1
                raise _Refuse("a lost suffix window of %d EST bytes" % elen)
            suf = (est[fl[1]:fl[1] + elen], gen[fl[3]:fl[3] + glen])
        else:
            info["suf_skipped"] = True
    recovered = 0
    for side, win in (("pre", pre), ("suf", suf)):
        if win is None:
            continue
        r = ops.affix(*win)
        for n in (64, 65, 256):
            if len(win[0]) == n:
                info["affix_%d" % n] = True
        info["dp_affix"] = info.get("dp_affix", 0) + 1
        if not r["valid"]:
            info[side + "_no_cut"] = True
            continue
        info[side + "_recovered"] = True
        if info.get("tagged") and _affix_tie(*win):
            info[side + "_tie"] = True
        if side == "pre":
            ff[0] -= r["ecut"]
            ff[2] -= r["gcut"]
            steps[0] |= STEP_PREFIX
            recovered |= 1
        else:
            fl[1] += r["ecut"]
            fl[3] += r["gcut"]
            steps[-1] |= STEP_SUFFIX
            recovered |= 2
    return recovered


def _ed(ops, a, b, info):
    """compute_edit_distance (src/compute-alignments.c:240-249): 0 without a dynamic program for equal strings"""
    if a == b:
        return 0
    info["dp_ed"] = info.get("dp_ed", 0) + 1
    return ops.ed(a, b)


def analyze_small_exon(est, gen, ex, prev, curr, nxt, ops, info):
    """analyze_possibly_small_exon (:960-1093) on the exons at the places prev, curr, nxt (None: there is none) ->
    the outcome; on REMOVED the four ends are moved"""
    if prev is None or nxt is None:
        return NOT_ANALYSED
    P, Cx, N = ex[prev], ex[curr], ex[nxt]
    elen, glen = Cx[1] + 1 - Cx[0], Cx[3] + 1 - Cx[2]
    if elen > UB_MED_EXON:
        if elen == UB_MED_EXON + 1:
            info["exon_101"] = True
        return NOT_ANALYSED
    if P[3] >= Cx[2] or Cx[3] >= N[2]:                       # an earlier merge with off_t1 > off_t2 lost the order
        return REFUSED
    estart = max(P[0] + 1, P[1] + 1 - AFFIXES_LENGTH)
    eend = min(N[1], N[0] + AFFIXES_LENGTH)
    epreflen, esufflen, allelen = P[1] + 1 - estart, eend - N[0], eend - estart
    gstart = max(P[2] + 1, P[3] + 1 - AFFIXES_LENGTH)
    gend = min(N[3], N[2] + AFFIXES_LENGTH)
    gpreflen, gsufflen, allglen = P[3] + 1 - gstart, gend - N[2], gend - gstart
    a0, b0 = est[Cx[0]:Cx[1] + 1], gen[Cx[2]:Cx[3] + 1]
    if allelen > MAX_SMALL_WINDOW and not info.get("no_caps"):
        info["window_129"] = info.get("window_129") or allelen == MAX_SMALL_WINDOW + 1
        raise _Refuse("a small-exon window of %d EST bytes" % allelen)
    if a0 != b0 and glen > MAX_SMALL_GEN and not info.get("no_caps"):
        info["gen_257"] = info.get("gen_257") or glen == MAX_SMALL_GEN + 1
        raise _Refuse("an analysed exon of %d genomic bytes" % glen)
    orig_ed = _ed(ops, a0, b0, info)
    ed_pref = _ed(ops, est[estart:estart + epreflen], gen[gstart:gstart + gpreflen], info)
    ed_suff = 0
    if estart >= esufflen and gstart >= gsufflen:            # the "suffix" pair IN FRONT of the window start (:1017-1018)
        ed_suff = _ed(ops, est[estart - esufflen:estart], gen[gstart - gsufflen:gstart], info)
    else:
        info["front_suffix"] = True
    max_errs = orig_ed + ed_pref + ed_suff
    info["dp_borders"] = info.get("dp_borders", 0) + 1
    r = ops.borders(est[estart:eend], gen, gstart, gend, max_errs)
    if elen == UB_MED_EXON:
        info["exon_100"] = True
    if allelen == MAX_SMALL_WINDOW:
        info["window_128"] = True
    if glen == MAX_SMALL_GEN and a0 != b0:
        info["gen_256"] = True
    if not r["ok"]:
        info["refine_refused"] = True
        return REFUSED
    off_p, off_t1, off_t2 = r["off_p"], r["off_t1"], r["off_t2"]
    old = KL.burset_adaptor(gen, P[3] + 1, Cx[2]) + KL.burset_adaptor(gen, Cx[3] + 1, N[2])
    new = KL.burset_adaptor(gen, gstart + off_t1, gend - allglen + off_t2)
    if not (new >= old / 2.0):
        info["burset_lower"] = True
        return BURSET_FELL
    if 2 * new == old and old > 0:
        info["burset_equal"] = True
    P[1] = estart + off_p - 1
    N[0] = eend + off_p - allelen
    P[3] = gstart + off_t1 - 1
    N[2] = gend + off_t2 - allglen
    return REMOVED


def remove_false_small_exons(est, gen, ex, steps, ops, info, reanalyse=True):
    """remove_false_small_exons (:1095-1125): the walk with prev / curr / next over the places of `ex`; a removed exon
    keeps its entry and gets REMOVED in its step byte.  `reanalyse=False` leaves the second look at the merged
    predecessor out (tools/make_tail_golden.py tries that once: the fixture must notice)."""
    n = len(ex)
    prev = curr = None
    nxt = 0
    removed = False
    last_removed = False
    while nxt is not None:
        if not removed:
            prev, curr = curr, nxt
            nxt = nxt + 1 if nxt + 1 < n else None
        outcome = analyze_small_exon(est, gen, ex, prev, curr, nxt, ops, info)
        removed = outcome == REMOVED
        if outcome != NOT_ANALYSED:
            steps[curr] = (steps[curr] & ~3) | outcome
        if removed:
            info["removed"] = True
            if curr == 1:
                info["removed_at_1"] = True
            if last_removed:
                info["removed_twice"] = True
            curr = prev                                      # :1077-1083
            prev = curr - 1
            while prev >= 0 and steps[prev] & 3 == REMOVED:
                prev -= 1
            prev = None if prev < 0 else prev
            if not reanalyse:
                removed = False                              # (the walk goes on from the merged exon as if it had been looked at)
        last_removed = outcome == REMOVED
    return sum(1 for s in steps if s & 3 != REMOVED)


def tail(orig: bytes, est: bytes, gen: bytes, exons, ops=ORACLE, info=None, reanalyse=True):
    """One query -> (status, verdict, polyA, polyadenil, recovered, n_kept, tail_added, exons afterwards, steps).  exons:
    [(EST_start, EST_end, GEN_start, GEN_end)], a query the entry accepts (einval); the exons afterwards and the steps are
    parallel to them.  `info` (a dict) receives what the fixture's cover counts; info["tagged"] asks for the tags that cost
    a second computation, info["no_caps"] lifts the caps of the entry (the host code has none)."""
    info = {} if info is None else info
    given = [tuple(int(v) for v in e) for e in exons]
    n = len(given)
    refused = (ERANGE, 0, 0, 0, 0, 0, 0, given, [0] * n)
    if n > MAX_EXONS and not info.get("no_caps"):
        info["refused"] = "more than %d exons" % MAX_EXONS
        info["exons_65"] = n == MAX_EXONS + 1
        return refused
    info["exons_64"] = n == MAX_EXONS
    info["orig_differs"] = orig != est
    ex = [list(e) for e in given]
    steps = [0] * n
    added = correct_tail(orig, gen, ex[-1])
    for k in (0, 63, 64, 65):
        info["ext_%d" % k] = added == k
    info["ext_to_est_end"] = added > 0 and ex[-1][1] == len(orig) - 1
    info["ext_to_gen_end"] = added > 0 and ex[-1][3] == len(gen) - 1
    polyA, polyadenil = detect_polyA(orig, gen, ex[-1], info)
    if invalid(ex, info):
        return OK, 1, int(polyA), int(polyadenil), 0, 0, added, [tuple(e) for e in ex], steps
    try:
        recovered = recover_affixes(est, gen, ex, steps, ops, info)
        kept = remove_false_small_exons(est, gen, ex, steps, ops, info, reanalyse)
    except _Refuse as why:
        info["refused"] = str(why)
        return refused
    if added:
        steps[-1] |= STEP_TAIL
    return OK, 0, int(polyA), int(polyadenil), recovered, kept, added, [tuple(e) for e in ex], steps


def kept_exons(answer):
    """the exons a caller goes on with: the ones step 5 did not remove"""
    return [e for e, s in zip(answer[7], answer[8]) if s & 3 != REMOVED]


def tags_of(info):
    return sorted(t for t in TAGS if info.get(t))


# ---- the PGPU_EINVAL rules ------------------------------------------------------------------------------------------
def einval(ests_len, gen_len, exons, queries):
    """True when pgpu_index_tail_chains refuses the whole call.  exons: array or list of 4-tuples; queries: records or
    dicts with the fields of pgpu_tail_query."""
    named = set()
    for q in queries:
        est_off, est_len, first, n = int(q["est_off"]), int(q["est_len"]), int(q["first_exon"]), int(q["n_exons"])
        orig_off = int(q["orig_off"])
        if est_off > ests_len or est_len > ests_len - est_off or est_len == 0 or est_len > 0x7FFFFFFF or int(q["reserved"]) != 0:
            return True
        if orig_off > ests_len or est_len > ests_len - orig_off:
            return True
        if n == 0 or first > len(exons) or n > len(exons) - first:
            return True
        for k in range(first, first + n):
            if k in named:
                return True
            named.add(k)
            es, ee, gs, ge = (int(v) for v in exons[k])
            if not (0 <= es < est_len and 0 <= ee < est_len and 0 <= gs < gen_len and 0 <= ge < gen_len):
                return True
    return False


# ---- hand-made cases --------------------------------------------------------------------------------------------------
GEN_LEN = 300_000
READ_ZONE = 230_000       # builders that write into the sequence do so in slots in front of this; the rest is read only
SLOT = 700
_ACGT = b"ACGT"


def other_base(c):
    """an upper-case base that differs from c in either case, and is no A"""
    return next(b for b in b"CGT" if b != (c & ~32))


class World:
    """the sequence under construction and the cases planted in it: (name, orig, est, exons)"""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.g = bytearray(RL.rnd(self.rng, GEN_LEN))
        self.g[-5:] = b"AATAA"                               # a hexamer cut short by the sequence's end
        self.next_free = 100
        self.cases = []

    def slot(self, size=SLOT):
        """the start of a region of `size` bytes that no other case touches"""
        at = self.next_free
        self.next_free += size
        assert self.next_free <= READ_ZONE
        return at

    def spot(self, room=4000):
        """a place in the read-only zone, `room` bytes from its end at least"""
        return int(self.rng.integers(READ_ZONE, GEN_LEN - room - 100))

    def clear_a(self, lo, hi):
        """no a / A in g[lo, hi) (a slot's bytes): nothing there extends or cancels a polyA by chance"""
        for i in range(lo, hi):
            if self.g[i] in b"aA":
                self.g[i] = b"CGT"[int(self.rng.integers(3))]

    def add(self, name, est, exons, orig=None):
        self.cases.append((name, bytes(est if orig is None else orig), bytes(est), [tuple(e) for e in exons]))


def chain(g, at, parts, flank=b"", trail=b""):
    """exons and what lies between them from g[at] on -> (est, exons, the place behind the last exon): an int is an exon
    of that many bases copied from g, a tuple (EST gap bytes, genomic gap length) a junction"""
    est, exons = bytearray(flank), []
    for part in parts:
        if isinstance(part, int):
            exons.append((len(est), len(est) + part - 1, at, at + part - 1))
            est += g[at:at + part]
            at += part
        else:
            gap, gap_t = part
            est += gap
            at += gap_t
    return est + trail, exons, at


def _differing(rng, byte):
    return bytes([other_base(byte)])


def _plain(w, n_exons=None, lens=(20, 90), introns=(60, 400)):
    rng = w.rng
    n = int(rng.integers(1, 6)) if n_exons is None else n_exons
    parts = []
    for k in range(n):
        parts.append(int(rng.integers(*lens)))
        if k + 1 < n:
            parts.append((b"", int(rng.integers(*introns))))
    return parts


def build_tail_cases(w):
    """step 1 and step 2: extensions, polyA, hexamers, the two cancelling loops"""
    rng, g = w.rng, w.g
    for rep in range(REPS):
        # extended by 0 / 63 / 64 / 65 bases, then a byte that differs
        for k in (0, 63, 64, 65, int(rng.integers(1, 200))):
            at = w.spot()
            est, ex, end = chain(g, at, _plain(w))
            est += g[end:end + k] + _differing(rng, g[end + k]) + RL.rnd(rng, int(rng.integers(0, 30)))
            w.add("ext_%d" % k, est, ex)
        # to the EST's end
        at = w.spot()
        est, ex, end = chain(g, at, _plain(w))
        w.add("ext_to_est_end", est + g[end:end + int(rng.integers(1, 100))], ex)
        # to the sequence's end (whose last bytes are AATAA)
        k = int(rng.integers(6, 120))
        ln = int(rng.integers(20, 60))
        at = GEN_LEN - k - ln
        est, ex, end = chain(g, at, [ln])
        w.add("ext_to_gen_end", est + g[end:] + RL.rnd(rng, int(rng.integers(1, 20))), ex)
        # ---- polyA over a slot of its own: the exon, then ten bytes behind it, free of A
        for kind in ("yes", "eight", "AATAAA", "ATTAAA", "aataaa", "attaaa", "mixed", "run6", "count7", "nine_no_a"):
            at = w.slot(450)
            w.clear_a(at, at + 400)
            ln = int(rng.integers(50, 90))
            end = at + 200 + ln
            if kind in ("AATAAA", "ATTAAA", "aataaa", "attaaa"):
                p = end - 6 - int(rng.integers(0, 34))
                g[p:p + 6] = kind.encode()
            if kind == "mixed":
                p = end - 6 - int(rng.integers(0, 34))
                g[p:p + 6] = [b"AaTAAA", b"aATAAA", b"ATTAAa", b"attAaa"][rep % 4]
            if kind == "run6":
                p = end - 9 + int(rng.integers(0, 12))
                g[p:p + 6] = b"AaAAaA"
            if kind == "count7":
                g[end:end + 10] = b"AAACAAACAA"
            parts = _plain(w, int(rng.integers(1, 4)), lens=(20, 60), introns=(60, 120))
            parts[-1] = ln
            first = sum(p if isinstance(p, int) else p[1] for p in parts[:-1])
            est, ex, e2 = chain(g, end - ln - first, parts)
            assert e2 == end
            tail_bytes = {"eight": b"AAAAaAAA", "nine_no_a": b"AAAAAAA" + b"CA"}.get(kind, b"aAAAAAAAA" + RL.rnd(rng, int(rng.integers(1, 9))))
            w.add("polyA_" + kind, est + tail_bytes, ex)
        # a hexamer cut short by the sequence's end: the tail exon ends inside the last five bytes
        k = int(rng.integers(0, 5))
        ln = int(rng.integers(20, 60))
        at = GEN_LEN - 1 - k - ln + 1
        est, ex, end = chain(g, at, [ln])
        w.add("hex_cut", est + b"A" * 14 + b"C", ex)


def build_invalid_cases(w):
    rng, g = w.rng, w.g
    for rep in range(REPS):
        for rule in ("est_exon", "gen_exon", "est_pair", "gen_pair"):
            est, ex, end = chain(g, w.spot(), _plain(w, int(rng.integers(2, 6))))
            k = int(rng.integers(len(ex)))
            ex = [list(e) for e in ex]
            if rule == "est_exon":
                ex[k][0], ex[k][1] = ex[k][1], ex[k][0]
            elif rule == "gen_exon":
                ex[k][2], ex[k][3] = ex[k][3], ex[k][2]
            elif rule == "est_pair":
                k = max(k, 1)
                ex[k][0] = ex[k - 1][1] - int(rng.integers(0, 3))
            else:
                k = max(k, 1)
                ex[k][2] = ex[k - 1][3] - int(rng.integers(0, 3))
            w.add("inv_" + rule, est + RL.rnd(rng, 5), ex)


def build_affix_cases(w):
    """step 4: prefixes and suffixes recovered, skipped, without a cut, with a tie in weight; windows of 64 / 65 / 256 / 257
    EST bytes.  `idx` below counts the bytes of a window from the exon outwards."""
    rng, g = w.rng, w.g
    for rep in range(REPS):
        for side in ("pre", "suf"):
            for kind in ("recovered", "skipped", "no_cut", "tie", "w64", "w65", "w256", "w257", "w257_skipped"):
                at = w.spot()
                parts = _plain(w, int(rng.integers(1, 4)))
                width = {"w64": 64, "w65": 65, "w256": 256, "w257": 257, "w257_skipped": 257}.get(kind, int(rng.integers(26, 60)))
                skipped = kind in ("skipped", "w257_skipped")
                if side == "pre":
                    # the flank in front of the first exon is the whole EST in front of it: a copy of the sequence there, idx 0
                    # substituted (so that the DP runs).  A tie: idx 0 and idx k substituted in a window of 2 k bytes, so that
                    # the cells (k, k) and (2 k, 2 k) weigh 1 / 2 k both
                    if kind == "tie":
                        k = int(rng.integers(6, 30))
                        width = 2 * k
                    flank = bytearray(g[at - width:at]) if kind != "no_cut" else bytearray(RL.rnd(rng, width))
                    if not skipped:
                        flank[-1] = other_base(g[at - 1])
                    if kind == "tie":
                        flank[-1 - k] = other_base(flank[-1 - k])
                    est, ex, end = chain(g, at, parts, flank=bytes(flank))
                    est += _differing(rng, g[end]) + RL.rnd(rng, 3)
                else:
                    # behind the last exon: idx 0 is the exon's last byte (the windows start ON it), substituted on the EST; idx 1
                    # is substituted too, so that step 1 adds nothing; then a copy of the sequence.  The window has as many
                    # bytes as the EST has behind the exon.  A tie: idx k and k + 1 substituted as well in a window of 2 k
                    # bytes: (k, k) and (2 k, 2 k) weigh 2 / 2 k both
                    if kind == "tie":
                        k = int(rng.integers(12, 30))
                        width = 2 * k
                    est, ex, end = chain(g, at, parts)
                    body = bytearray(g[end:end + width]) if kind != "no_cut" else bytearray(RL.rnd(rng, width))
                    body[0] = other_base(g[end])
                    if kind == "tie":
                        body[k - 1] = other_base(body[k - 1])
                        body[k] = other_base(body[k])
                    if not skipped:
                        est[-1] = other_base(est[-1])
                    est += body
                w.add("%s_%s" % (side, kind), est, ex)


def _false_small(w, at, lens, sites, x_len, gap=(b"", b""), prev_len=None, c_end=None):
    """[prev][GT .. AG][X][GT .. AG][C N] over the slot at `at`, X a copy of C, the bytes in front of the true exon C N:
    the factorization (prev, X, N) has a false small exon X.  sites: (donor1, acceptor1, donor2, what stands in front of C,
    i.e. the new intron's acceptor); c_end: the last bytes of C, and so of X.  Returns (est, exons)."""
    rng, g = w.rng, w.g
    lp = int(rng.integers(20, 60)) if prev_len is None else prev_len
    i1, i2, ln = lens
    d1, a1, d2, a_new = sites
    p0 = at
    x0 = p0 + lp + i1
    c0 = x0 + x_len + i2
    n0 = c0 + x_len
    g[p0 + lp:p0 + lp + 2] = d1
    g[x0 - 2:x0] = a1
    g[x0 + x_len:x0 + x_len + 2] = d2
    g[c0 - 2:c0] = a_new
    if c_end:
        g[c0 + x_len - len(c_end):c0 + x_len] = c_end
    g[x0:x0 + x_len] = g[c0:c0 + x_len]
    est = bytes(g[p0:p0 + lp]) + gap[0] + bytes(g[x0:x0 + x_len]) + gap[1] + bytes(g[n0:n0 + ln])
    e1 = lp + len(gap[0])
    e2 = e1 + x_len + len(gap[1])
    return est, [(0, lp - 1, p0, p0 + lp - 1), (e1, e1 + x_len - 1, x0, x0 + x_len - 1), (e2, e2 + ln - 1, n0, n0 + ln - 1)]


def build_small_cases(w):
    """step 5"""
    rng, g = w.rng, w.g
    for rep in range(REPS):
        for kind in ("removed", "equal", "lower", "refused", "at_1_head", "front", "e100", "e101", "w128", "w129", "g256", "g257", "twice"):
            at = w.slot()
            lens = (int(rng.integers(80, 200)), int(rng.integers(80, 200)), int(rng.integers(20, 60)))
            x_len = int(rng.integers(6, 16))
            gt_ag = (b"GT", b"AG", b"GT", b"AG")
            if kind == "removed":
                est, ex = _false_small(w, at, lens, (b"CC", b"CC", b"CC", b"CC"), x_len)
            elif kind == "equal":                               # X (and so C) ends in AG: 2 x 200 against 200 + 200
                est, ex = _false_small(w, at, lens, gt_ag, x_len, c_end=b"AG")
            elif kind == "lower":
                est, ex = _false_small(w, at, lens, (b"GT", b"AG", b"GT", b"CC"), x_len)
            elif kind == "refused":                             # X is no copy of anything near N
                est, ex = _false_small(w, at, lens, gt_ag, x_len)
                g[ex[1][2]:ex[1][3] + 1] = RL.rnd(rng, x_len)
                est = est[:ex[1][0]] + bytes(g[ex[1][2]:ex[1][3] + 1]) + est[ex[1][1] + 1:]
            elif kind == "at_1_head":
                est, ex = _false_small(w, at, lens, (b"CC", b"CC", b"CC", b"CC"), x_len, prev_len=int(rng.integers(12, 30)))
            elif kind == "front":                               # a first exon of at most nine bytes at the EST's first byte
                est, ex = _false_small(w, at, lens, (b"CC", b"CC", b"CC", b"CC"), x_len, prev_len=int(rng.integers(2, 9)))
            elif kind in ("e100", "e101"):
                est, ex = _false_small(w, at, (150, 150, 30), (b"CC", b"CC", b"CC", b"CC"), 100 if kind == "e100" else 101)
            elif kind in ("w128", "w129"):                      # 5 + gaps + 100 + 5
                total = 18 if kind == "w128" else 19
                k = int(rng.integers(0, total + 1))
                est, ex = _false_small(w, at, (150, 150, 30), (b"CC", b"CC", b"CC", b"CC"), 100,
                                       gap=(RL.rnd(rng, k), RL.rnd(rng, total - k)))
            elif kind in ("g256", "g257"):                      # an exon of 90 EST bytes over 256 / 257 genomic ones
                n_g = 256 if kind == "g256" else 257
                lp, ln = 30, 30
                x0 = at + lp + 150
                n0 = x0 + n_g + 150
                est = bytes(g[at:at + lp]) + bytes(g[x0:x0 + 45]) + bytes(g[x0 + n_g - 45:x0 + n_g]) + bytes(g[n0:n0 + ln])
                ex = [(0, lp - 1, at, at + lp - 1), (lp, lp + 89, x0, x0 + n_g - 1), (lp + 90, lp + 90 + ln - 1, n0, n0 + ln - 1)]
            else:                                               # twice: [P0] .. [Y copy] .. [X copy] .. [Y C N]
                y_len = int(rng.integers(6, 14))
                l0 = int(rng.integers(20, 50))
                y0 = at + l0 + int(rng.integers(80, 160))
                x0 = y0 + y_len + int(rng.integers(80, 160))
                t0 = x0 + x_len + int(rng.integers(80, 160))         # the true exon Y C N
                ln = lens[2]
                g[y0:y0 + y_len] = g[t0:t0 + y_len]
                g[x0:x0 + x_len] = g[t0 + y_len:t0 + y_len + x_len]
                n0 = t0 + y_len + x_len
                est = bytes(g[at:at + l0]) + bytes(g[y0:y0 + y_len]) + bytes(g[x0:x0 + x_len]) + bytes(g[n0:n0 + ln])
                a, b = l0 + y_len, l0 + y_len + x_len
                ex = [(0, l0 - 1, at, at + l0 - 1), (l0, a - 1, y0, y0 + y_len - 1), (a, b - 1, x0, x0 + x_len - 1), (b, b + ln - 1, n0, n0 + ln - 1)]
            end = ex[-1][3] + 1
            w.add("small_" + kind, est + _differing(rng, g[end]) + RL.rnd(rng, 2), ex)


def build_other_cases(w):
    rng, g = w.rng, w.g
    for rep in range(REPS):
        for n in (64, 65):
            parts = []
            for k in range(n):
                parts.append(int(rng.integers(3, 9)))
                if k + 1 < n:
                    parts.append((b"", int(rng.integers(30, 50))))
            est, ex, end = chain(g, w.spot(8000), parts)
            w.add("exons_%d" % n, est + _differing(rng, g[end]), ex)
        # the working sequence is the original with its ends masked
        est, ex, end = chain(g, w.spot(), _plain(w, int(rng.integers(1, 4))), flank=b"T" * int(rng.integers(8, 20)))
        orig = est + b"A" * int(rng.integers(9, 20)) + b"C"
        k = ex[0][0]
        work = b"#" * k + orig[k:len(est)] + b"*" * (len(orig) - len(est))
        w.add("orig_differs", work, ex, orig=orig)


def make_world(seed):
    """(the sequence, [(name, orig, est, exons)]): the hand-made cases of every builder"""
    w = World(seed)
    build_small_cases(w)              # (first: the slots of these cases are the widest users of the write zone)
    build_tail_cases(w)
    build_invalid_cases(w)
    build_affix_cases(w)
    build_other_cases(w)
    return bytes(w.g), w.cases


def generated(seed, gen: bytes, n):
    """n fresh ordinary factorizations over `gen`, read only: one to six exons copied from the read-only zone, now and then
    a substituted base, random flanks, and behind the last exon a few bytes of the sequence, a polyA or nothing"""
    rng = np.random.default_rng(seed)
    out = []

    class _W:
        pass
    w = _W()
    w.rng = rng
    for _ in range(n):
        at = int(rng.integers(READ_ZONE, len(gen) - 6000))
        parts = _plain(w, int(rng.integers(1, 7)), lens=(4, 120), introns=(40, 300))
        flank = RL.rnd(rng, int(rng.integers(0, 40))) if rng.random() < 0.6 else b""
        if rng.random() < 0.3 and at > 60:
            k = int(rng.integers(8, 50))
            flank = bytes(gen[at - k:at - 1]) + bytes([other_base(gen[at - 1])])
        est, ex, end = chain(gen, at, parts, flank=flank)
        est = bytearray(est)
        for _k in range(int(rng.integers(0, 3))):
            p = int(rng.integers(len(est)))
            est[p] = _ACGT[int(rng.integers(4))]
        r = rng.random()
        if r < 0.3:
            est += gen[end:end + int(rng.integers(1, 80))] + RL.rnd(rng, int(rng.integers(0, 10)))
        elif r < 0.6:
            est += b"A" * int(rng.integers(6, 14)) + RL.rnd(rng, int(rng.integers(0, 4)))
        elif r < 0.8:
            est += RL.rnd(rng, int(rng.integers(1, 40)))
        out.append(("generated", bytes(est), bytes(est), ex))
    return out


# ---- the arrays of the entry ------------------------------------------------------------------------------------------
def batch_arrays(cases):
    """cases of (name, orig, est, exons) -> (ests, exons array, queries array) in the layouts of the entry; equal strings
    are stored once"""
    from pintron_amd import capi
    n_ex = sum(len(c[3]) for c in cases)
    exons = np.zeros(n_ex, dtype=np.dtype(capi.FACTOR_DTYPE))
    q = np.zeros(len(cases), dtype=np.dtype(capi.TAIL_QUERY_DTYPE))
    ests, eat, k = [], {}, 0
    size = 0
    for i, (_, orig, est, ex) in enumerate(cases):
        for s in (est, orig):
            if s not in eat:
                eat[s] = size
                ests.append(s)
                size += len(s)
        for e in ex:
            exons[k] = tuple(e)
            k += 1
        q[i] = (eat[est], len(est), k - len(ex), len(ex), 0, eat[orig])
    return b"".join(ests), exons, q


def expect_arrays(exons, answers):
    """answers of tail() per query, in the order of the exons -> the three arrays of the entry"""
    from pintron_amd import capi
    out_exons = exons.copy()
    out_steps = np.zeros(len(exons), dtype=np.uint8)
    res = np.zeros(len(answers), dtype=np.dtype(capi.TAIL_RESULT_DTYPE))
    k = 0
    for i, (status, verdict, polyA, polyadenil, recovered, kept, added, ex2, steps) in enumerate(answers):
        res[i] = (status, verdict, polyA, polyadenil, recovered, kept, added)
        for e, s in zip(ex2, steps):
            out_exons[k] = tuple(e)
            out_steps[k] = s
            k += 1
    assert k == len(exons)
    return out_exons, out_steps, res


def _case_dicts(rows):
    cases = []
    for name, orig, est, ex, res, after, steps, tags in rows:
        est = est.encode()
        cases.append(dict(name=name, orig=est if orig is None else orig.encode(), est=est, exons=[tuple(e) for e in ex],
                          answer=tuple(res) + ([tuple(e) for e in after], list(steps)), tags=set(tags)))
    return cases


_fixture = []


def load_fixture():
    """(genomic bytes, [case dicts: name, orig, est, exons, answer (the tuple of tail()), tags], {source: [case dicts]}):
    the hand-made cases over the seeded sequence, and the ones of the real inputs (over their own sequences: real_genomic)"""
    if not _fixture:
        doc = json.load(gzip.open(FIXTURE, "rt"))
        g = bytearray(RL.rnd(np.random.default_rng(doc["seed"]), doc["length"]))
        for pos, s in doc["edits"]:
            g[pos:pos + len(s)] = s.encode()
        _fixture.append((bytes(g), _case_dicts(doc["cases"]), {src: _case_dicts(rows) for src, rows in doc["real"].items()}))
    return _fixture[0]


def quads(cases):
    return [(c["name"], c["orig"], c["est"], c["exons"]) for c in cases]


# ---- today's device route ---------------------------------------------------------------------------------------------
class _Asked(Exception):
    pass


class _DeviceOps:
    """answers from the plans run so far; a question without one is noted, and the query that asked waits for the next round"""

    def __init__(self):
        self.got, self.want = {}, {}

    def _ask(self, key):
        if key in self.got:
            return self.got[key]
        self.want.setdefault(key, len(self.want))
        raise _Asked()

    def affix(self, e, g):
        return self._ask(("affix", e, g))

    def ed(self, a, b):
        return self._ask(("ed", a, b))["score"]

    def borders(self, p, gen, gstart, gend, max_errs):
        return self._ask(("borders", p, gstart, gend, max_errs))


def device_route(ctx, idx, gen: bytes, cases, clock=None):
    """cases of (name, orig, est, exons) -> the answers of tail(), every question asked of the device as a PGPU_DP_AFFIX,
    PGPU_DP_ED or PGPU_DP_BORDERS job (the last with PGPU_JOB_B_GENOMIC and the bytes behind the window as its tail) of one
    plan per round -- an analysis needs its edit distances before its refinement, and a merged exon its neighbours' ends --
    with the glue of tail() on the host.  `clock` (a dict) receives "library_s", the seconds inside the plans' entry
    points, "jobs" and "rounds"."""
    import ctypes as C
    import time
    from pintron_amd import capi
    ops = _DeviceOps()
    L = ctx.L
    inside, n_jobs, rounds = 0.0, 0, 0
    answers = [None] * len(cases)
    while True:
        for k, (_, orig, est, ex) in enumerate(cases):
            if answers[k] is None:
                try:
                    answers[k] = tail(orig, est, gen, ex, ops=ops)
                except _Asked:
                    pass
        if not ops.want:
            break
        keys = sorted(ops.want, key=ops.want.get)
        jl = capi.JobList()
        for key in keys:
            if key[0] == "affix":
                jl.add(capi.AFFIX, key[1], key[2])
            elif key[0] == "ed":
                jl.add(capi.ED, key[1], key[2])
            else:
                _, p, gstart, gend, max_errs = key
                jl.add(capi.BORDERS, p, bytes(gend - gstart), p0=0, p1=len(p), p2=max_errs, b_gen_off=gstart,
                       tail=min(2, len(gen) - gend))
        jobs, arena = jl.arrays()
        n = len(jl.jobs)
        res = (capi.DpResult * n)()
        h = C.c_void_p()
        t0 = time.perf_counter()
        rc = L.pgpu_dp_plan_create(ctx.h, idx.h, jobs, n, arena, len(arena), C.byref(h))
        inside += time.perf_counter() - t0
        ctx.check(rc)
        try:
            t0 = time.perf_counter()
            rc = L.pgpu_dp_plan_launch(ctx.h, h) or L.pgpu_dp_plan_sync(ctx.h, h)
            nbytes = L.pgpu_dp_plan_string_bytes(h)
            sbuf = C.create_string_buffer(max(nbytes, 1))
            rc = rc or L.pgpu_dp_plan_fetch(ctx.h, h, res, sbuf, nbytes)
            inside += time.perf_counter() - t0
            ctx.check(rc)
        finally:
            t0 = time.perf_counter()
            L.pgpu_dp_plan_destroy(ctx.h, h)
            inside += time.perf_counter() - t0
        kinds = {"affix": capi.AFFIX, "ed": capi.ED, "borders": capi.BORDERS}
        for key, r in zip(keys, res):
            o = capi.decode(kinds[key[0]], r, b"")
            assert o["status"] == 0, o
            ops.got[key] = o
        ops.want = {}
        n_jobs += n
        rounds += 1
    if clock is not None:
        clock["library_s"], clock["jobs"], clock["rounds"] = inside, n_jobs, rounds
    return answers


# ---- the host's own routines: ef_chain_tail, the oracle as backend (ef_gpu_open over tests/hostcheck/fake_pgpu.c) ------
class Host:
    def __init__(self, genomic: bytes):
        import ctypes as C
        import struct
        H = self.H = KL.host_lib()
        H.ef_gpu_open.restype = C.c_void_p
        H.ef_gpu_open.argtypes = [C.c_void_p]
        H.ef_gpu_close.argtypes = [C.c_void_p]
        H.ef_chain_factorization.restype = C.c_uint
        H.ef_chain_factorization.argtypes = [C.c_char_p, C.c_void_p, C.c_char_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                             C.POINTER(C.c_uint)]
        H.ef_chain_tail.restype = C.c_uint
        H.ef_chain_tail.argtypes = [C.c_char_p, C.c_char_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint] + [C.POINTER(C.c_uint)] * 3
        self.gen = C.create_string_buffer(genomic, len(genomic) + 2)
        self.seq = C.create_string_buffer(4096)                   # an ef_seq: char* id, seq, original_seq, ...; the rest 0
        struct.pack_into("<QQQ", self.seq, 0, 0, C.addressof(self.gen), C.addressof(self.gen))
        self.cfg = C.create_string_buffer(4096)
        H.ef_config_defaults(self.cfg)
        self.be = H.ef_gpu_open(self.seq)
        assert self.be

    def factorization(self, rec, est: bytes):
        """ef_chain_factorization: (0 not one path | 1 no factorization | 2, exons)"""
        import ctypes as C
        cap = 128
        ex = (C.c_int32 * (4 * cap))()
        n = C.c_uint(0)
        kind = self.H.ef_chain_factorization(rec, self.cfg, est, self.gen, self.be, ex, cap, C.byref(n))
        assert n.value <= cap
        return kind, [tuple(ex[4 * k:4 * k + 4]) for k in range(n.value)]

    def tail(self, orig: bytes, est: bytes, exons):
        """ef_chain_tail -> (verdict, polyA, polyadenil, the exons left; on verdict 1 the exons as correct_tail left them)"""
        import ctypes as C
        n = len(exons)
        ex = (C.c_int32 * (4 * n))(*[v for e in exons for v in e])
        n_out, pa, pn = C.c_uint(0), C.c_uint(0), C.c_uint(0)
        dropped = self.H.ef_chain_tail(est, orig, self.gen, self.be, ex, n, C.byref(n_out), C.byref(pa), C.byref(pn))
        return dropped, pa.value, pn.value, [tuple(ex[4 * k:4 * k + 4]) for k in range(n_out.value)]

    def close(self):
        self.H.ef_gpu_close(self.be)


def agrees_with_host(answer, host_answer):
    """what ef_chain_tail can say of one accepted query, against the restatement's answer"""
    status, verdict, polyA, polyadenil, recovered, kept, added, after, steps = answer
    assert status == OK
    want = after if verdict else kept_exons(answer)
    return host_answer == (verdict, polyA, polyadenil, want)


_real = {}


def real_done(source):
    """(genomic, [(est, exons)]): the DONE factorizations ef_chain_factorization gives on one real input ("c2", "ambn",
    "issue13") under the defaults, the host's graphs; computed once"""
    if source not in _real:
        import meg_lib as M
        gfa, efa = KL.real_inputs()[source]
        exp, genomic = M.first_attempt_megs(gfa, efa, M.DEFAULTS)
        recs, _ = KL.host_records(gfa, efa, M.DEFAULTS)
        host = Host(genomic)
        out = []
        try:
            for e, rec in zip(exp, recs):
                est = e["seq"].encode() if isinstance(e["seq"], str) else e["seq"]
                kind, exons = host.factorization(rec, est)
                if kind == 2:
                    out.append((est, exons))
        finally:
            host.close()
        _real[source] = (genomic, out)
    return _real[source]
