"""Edge cases of the pairing kernels (pgpu_pairing_plan.hip): small min_factor_len, matches laid against the 16- and
32-base words of the packed sequences, flagged bases (N, lower case, the '*' and '#' of the poly-A/T masks), byte order
in the suffix array, thresholds that hang on the double's truncation, crowded position lists, odd batches.

One seeded generator per group, each returning [(name, genomic, [est, ...], [(L, rate), ...])], and one tag function
per group, which decides from a case's inputs and the oracle's answer (pairings and the locus depths D_i) what the case
reached.  tools/make_pairing_edges_golden.py writes the committed fixture from seed FIXTURE_SEED; the GPU tests draw
fresh cases from other seeds."""
import json
import os
import random
import subprocess
import sys
from fractions import Fraction

import pairing_lib as PL

GROUPS = ("small_L", "windows", "flagged", "order", "threshold", "crowded", "batch")
FIXTURE_SEED = 1
ACGT = b"ACGT"
RES = (0, 1, 15, 16, 17, 31)                                    # residues mod 32 of a match's two offsets
LENS = (15, 16, 17, 31, 32, 33, 47, 48, 63, 64, 65)
SMALL_LS = (1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 32, 33, 48, 64)
FLAG_BYTES = b"Nna*#"
ORDER_ALPHABET = b"#*ACGNTacgt"
# Two places where the reference's object code dies whatever the genome, found while the fixture was made: every query
# at min_factor_len 1, and a position whose match begins with a byte that the genome holds once (the leaf hangs from the
# root).  The L = 1 cases stay, answered by the oracle alone, and the cover counts them apart; a flagged byte that begins
# a match is given a second occurrence on the genome's last base, away from the match, so that the reference answers.
REFERENCE_DIES_AT_L = (1,)
UNIQUE_FIRST_BYTE = "a match beginning with a byte the genome holds once"
THRESHOLDS = ((100, 0.29), (50, 0.58), (100, 0.57))             # D * rate just below an integer, in double


def _rng(group, seed):
    return random.Random(seed * 16 + GROUPS.index(group))


def rs(rng, n, al=ACGT):
    return bytes(rng.choices(al, k=n)) if n else b""


def other(rng, *avoid):
    """an upper-case base that differs from every given byte (and from its other case)"""
    bad = {bytes([c]).upper()[0] for c in avoid}
    return rng.choice([c for c in ACGT if c not in bad])


def _off(r):
    return r if r else 32                                        # residue 0 with a flanking base in front


def planted(rng, t, offsets, ln, g_tail=9, e_tails=(9,)):
    """A genomic sequence holding `core` (ln random bases) at t, and one EST per entry of `offsets` holding it at that
    offset; the bases in front of and behind the match differ between the two sequences (where both have one)."""
    core = rs(rng, ln)
    gl, gr = bytearray(rs(rng, t)), bytearray(rs(rng, g_tail))
    ests = []
    for k, i in enumerate(offsets):
        el, er = bytearray(rs(rng, i)), bytearray(rs(rng, e_tails[k % len(e_tails)]))
        if el and gl and el[-1] == gl[-1]:
            el[-1] = other(rng, gl[-1])
        if er and gr and er[0] == gr[0]:
            er[0] = other(rng, gr[0])
        ests.append(bytes(el) + core + bytes(er))
    return bytes(gl) + core + bytes(gr), ests


# ---- the groups --------------------------------------------------------------------------------------------------

def small_L(seed):
    rng = _rng("small_L", seed)
    out = []
    for L in SMALL_LS:
        n = 600 if L <= 3 else 3000
        g = bytearray(rs(rng, n))
        span = max(2 * L + 8, 24) if L <= 3 else max(3 * L, 60)
        a = rng.randint(50, n // 2 - span)
        g[n - 40 - span:n - 40] = PL.revcomp(bytes(g[a:a + span]))          # so that reverse complements match too
        gen = bytes(g)
        subs = []
        for k in range(4):
            s = rng.randint(0, n - span - 1) if k else a
            e = bytearray(gen[s:s + span])
            for _ in range(k):                                                # 0..3 substitutions
                q = rng.randrange(len(e))
                e[q] = other(rng, e[q])
            subs.append(bytes(e))
        s = rng.randint(1, n - L - 2)
        exact = [gen[s:s + L - 1], gen[s:s + L], gen[s:s + L + 1]]
        absent = []
        if L >= 7:                                                            # a first L-mer that does not occur
            while True:
                head = rs(rng, min(L, 8))
                if head not in gen:
                    break
            absent = [head + gen[s:s + span], head]
        ests = subs + [PL.revcomp(e) for e in subs] + exact + absent
        if L <= 3:      # nearly every occurrence of a base pairs at rate 0.2: few ESTs there, all of them at rate 1.0
            out.append(("small_L/L%d/dense" % L, gen, subs[:2] + exact, [(L, 0.2)]))
            out.append(("small_L/L%d" % L, gen, ests, [(L, 1.0)]))
        else:
            out.append(("small_L/L%d" % L, gen, ests, [(L, 0.2), (L, 0.5)]))
    return out


def windows(seed):
    rng = _rng("windows", seed)
    out = []
    for tr in RES:
        for ln in LENS:
            gen, ests = planted(rng, _off(tr), [_off(ir) for ir in RES], ln)
            out.append(("windows/t%d/len%d" % (tr, ln), gen, ests, [(15, 0.2)]))
    for b, ln in enumerate(LENS):
        tr = RES[b % len(RES)]
        offs = [_off(ir) for ir in RES]
        # the match ends on the last base of the genome; the ESTs end there too, or run on for 1, 9 or 40 bases
        gen, ests = planted(rng, _off(tr), offs, ln, g_tail=0, e_tails=(0, 1, 9, 40))
        out.append(("windows/gend/t%d/len%d" % (tr, ln), gen, ests, [(15, 0.2)]))
        # the match ends on the last base of every EST: of the batch's last pattern, and of patterns with others behind
        gen, ests = planted(rng, _off(tr), offs, ln, e_tails=(0,))
        out.append(("windows/eend/t%d/len%d" % (tr, ln), gen, ests, [(15, 0.2)]))
        # the match starts both sequences
        gen, ests = planted(rng, 0, [0, 1, 16], ln)
        out.append(("windows/start/len%d" % ln, gen, ests, [(15, 0.2)]))
    return out


def _flag_modes(byte):
    """(mode, byte in the genome, byte in the EST); None = an ordinary base"""
    plain = ord("A") if byte == ord("a") else None
    return [("gen", byte, plain), ("est", plain, byte), ("both", byte, byte)]


def flagged(seed):
    rng = _rng("flagged", seed)
    out = []
    k = 0
    for byte in FLAG_BYTES:
        for o_name in (0, 7, 8, 15, 16, "last"):
            for rot in range(2):
                ln = (33, 48, 65, 32)[(k + rot) % 4]
                o = ln - 1 if o_name == "last" else o_name
                t, i = _off(RES[k % 6]), _off(RES[(k // 6 + rot) % 6])
                k += 1
                for mode, gb, eb in _flag_modes(byte):
                    gen, (est,) = planted(rng, t, [i], ln)
                    g, e = bytearray(gen), bytearray(est)
                    base = other(rng)
                    g[t + o] = gb if gb is not None else base
                    e[i + o] = eb if eb is not None else (other(rng, base) if mode != "both" else base)
                    if byte == ord("a") and mode != "both":                  # A against a: equal but for the case
                        g[t + o], e[i + o] = (gb, ord("A")) if mode == "gen" else (ord("A"), eb)
                    if mode == "both" and o == 0:
                        g[-1] = byte                                          # see UNIQUE_FIRST_BYTE
                    out.append(("flagged/%s/%d/o%s/len%d/t%d/i%d" % (mode, byte, o_name, ln, t, i), bytes(g), [bytes(e)],
                                [(15, 0.2)]))
    for byte in FLAG_BYTES:             # the byte inside the first 8 bases of the genome, and of the EST: no k-mer code
        for o in (0, 3, 7):
            gen, ests = planted(rng, 0, [0, 5], 40)
            g, es = bytearray(gen), [bytearray(e) for e in ests]
            g[o] = byte
            if o == 0:
                g[-1] = byte                                                  # see UNIQUE_FIRST_BYTE
            es[0][o] = byte
            es[1][5 + o] = byte
            out.append(("flagged/head/%d/o%d" % (byte, o), bytes(g), [bytes(e) for e in es], [(15, 0.2), (8, 0.2)]))
    left, mid, right = rs(rng, 200), rs(rng, 40), rs(rng, 200)
    gen = left + b"*" * 40 + right
    span = gen[150:300]
    out.append(("flagged/stretch/star", gen, [span, span.replace(b"*", b"#"), span.replace(b"*", b"N"), span.replace(b"*", b"A"),
                                              gen[190:260], gen[225:300], PL.revcomp(span)], [(15, 0.2), (8, 0.5)]))
    gen = left + mid.lower() + right
    span = gen[150:300]
    out.append(("flagged/stretch/lower", gen, [span, span.upper(), span.lower(), gen[190:260], gen[205:235], gen[205:235].upper(),
                                               PL.revcomp(span)], [(15, 0.2), (8, 0.5)]))
    return out


def order(seed, n_cases=48):
    """PL.region_start_cases over alphabets that hold bytes below 'A' and above 'T': the order of the suffix array, the
    comparison c < e of the bisection and, through the copies of t == 0, alphabet keys up to 10."""
    rng = _rng("order", seed)
    out = []
    for k in range(n_cases):
        al = rng.choice([ORDER_ALPHABET, ORDER_ALPHABET, b"#*ACGT", b"ACGTacgt", b"*ACGNT", b"#Aa", b"*#", b"ACGTn#"])
        head, x = rs(rng, 60, al), rs(rng, 120, al)
        rep = rng.choice([20, 40, 55])
        gen = head + rs(rng, rng.choice([5, 250]), al) + rs(rng, 1, al) + head[:rep] + x + rs(rng, 200, al)
        if rng.random() < 0.3:
            gen += head[:35] + rs(rng, 50, al)
        gen = gen[:900]
        ests = []
        for lead in (0, 1, 30):
            est = rs(rng, lead, ORDER_ALPHABET) + head[:rep] + x[:rng.choice([60, 100])]
            if rng.random() < 0.3 and len(est) > 60:
                est = est[:50] + rs(rng, 1, al) + est[51:]
            ests.append(est)
        out.append(("order/%d/%s" % (k, al.decode()), gen, ests, [(15, 0.2), (18, 0.1)]))
    return out


def _threshold_case(rng, D, rate, L=15):
    """An EST position whose locus has depth D, and occurrences of its first k - 1, k and k + 1 characters elsewhere,
    k = (uint32_t) max(D * rate, L) as the double gives it."""
    k = max(int(float(D) * rate), L)
    x = rs(rng, D)
    pre = other(rng)                                                          # the EST's base in front of x

    def piece(ln):                                                            # x[:ln], not prev-excluded, ending in a mismatch
        return rs(rng, rng.randint(20, 40)) + bytes([other(rng, pre)]) + x[:ln] + bytes([other(rng, x[ln])])

    nxt = other(rng)                                                          # the genome's base behind x
    gen = rs(rng, rng.randint(3, 70)) + bytes([other(rng, pre)]) + x + bytes([nxt])
    for ln in (k - 1, k, k + 1):
        if L <= ln < D:
            gen += piece(ln)
    gen += rs(rng, 30)
    est = rs(rng, rng.randint(1, 12)) + bytes([pre]) + x
    return gen, [est, est + bytes([other(rng, nxt)]) + rs(rng, 19)]


def threshold(seed):
    rng = _rng("threshold", seed)
    out = []
    for D, rate in THRESHOLDS:
        for k in range(3):
            gen, ests = _threshold_case(rng, D, rate)
            out.append(("threshold/D%d/r%s/%d" % (D, rate, k), gen, ests, [(15, rate)]))
    for D, rate in ((100, 0.0), (60, 0.25), (64, 0.25), (100, 0.999), (100, 1.0), (100, 1.5), (40, 0.999)):
        gen, ests = _threshold_case(rng, D, rate)
        out.append(("threshold/D%d/r%s/0" % (D, rate), gen, ests, [(15, rate)]))
    return out


def crowded(seed, n=20000, copies=80, unit_len=150):
    """A unit planted `copies` times, one copy at position 0, the others behind differing bases; inside it a run of 20 A
    between two other bases, which an EST with 21 A and other neighbours pairs with twice from the same t: filter (b)."""
    rng = _rng("crowded", seed)
    u = bytearray(rs(rng, unit_len))
    u[99] = rng.choice(b"CGT")
    u[100:120] = b"A" * 20
    u[120] = rng.choice(b"CGT")
    unit = bytes(u)
    g = bytearray(rs(rng, n))
    slot = (n - unit_len) // copies
    starts = [0] + [k * slot + rng.randint(1, slot - unit_len - 1) for k in range(1, copies)]
    for k, s in enumerate(starts):
        g[s:s + unit_len] = unit
        if s:
            g[s - 1] = ACGT[k % 4]
    gen = bytes(g)
    c = starts[rng.randint(2, copies - 2)]
    flank = bytearray(gen[c - 50:c + unit_len + 50])
    behind_n = bytes(flank[:49]) + b"N" + bytes(flank[50:])                   # no copy is prev-excluded
    runs = bytearray(flank)                                                    # 21 A between two substituted bases
    runs[50 + 99] = other(rng, unit[99], ord("A"))
    runs[50 + 120] = other(rng, unit[120], ord("A"))
    runs = bytes(runs[:50 + 100]) + b"A" + bytes(runs[50 + 100:])
    ests = [bytes(flank), behind_n, runs, unit + gen[c + unit_len:c + unit_len + 40], gen[:unit_len + 40], PL.revcomp(bytes(flank))]
    return [("crowded/%d" % seed, gen, ests, [(15, 0.2)])]


BATCH_LS = (7, 33, 8, 15, 2, 15)                                            # the order one plan of `batch` is rerun in


def batch(seed):
    """Plans of 63, 64, 65 and 129 patterns over a 600-base genome (short enough for L = 2); pattern lengths 0, 1, L - 1,
    L, 63, 64, 65, 127, 128, 129 and 2 000, empty patterns first, last and two in a row."""
    rng = _rng("batch", seed)
    gen = rs(rng, 600)

    def pattern(ln):
        e = bytearray()
        while len(e) < ln:                                                    # pieces of the genome, a substitution between them
            a = rng.randrange(len(gen))
            e += gen[a:a + rng.randint(10, 120)]
            e[-1] = other(rng, e[-1])
        return bytes(e[:ln])

    out = []
    for n_pat in (63, 64, 65, 129):
        lens = [0, 1, 2, 6, 7, 8, 14, 15, 32, 33, 63, 64, 65, 127, 128, 129] + ([2000] if n_pat == 129 else [])
        ests = [pattern(rng.choice(lens[:-1]) if k >= len(lens) else lens[k]) for k in range(n_pat - 5)]
        rng.shuffle(ests)
        ests = [b""] + ests[:20] + [b"", b""] + ests[20:] + [gen[:33], b""]
        assert len(ests) == n_pat
        out.append(("batch/%d" % n_pat, gen, ests, [(15, 0.2), (7, 0.2), (33, 0.2), (8, 0.2)]))
    return out


GENERATORS = dict(small_L=small_L, windows=windows, flagged=flagged, order=order, threshold=threshold, crowded=crowded,
                  batch=batch)


def cases(group, seed=FIXTURE_SEED):
    return GENERATORS[group](seed)


def fresh_cases(group, n, first_seed=1000):
    """n cases of the group from seeds the fixture does not hold"""
    out, seed = [], first_seed
    while len(out) < n:
        out += GENERATORS[group](seed)
        seed += 1
    return out[:n]


# ---- the oracle's answer -------------------------------------------------------------------------------------------

def oracle_answers(gen, ests, params, depths=False):
    """[[pairings of est (n x 3 array), ...] per (L, rate)]; with depths, (pairings, D) pairs"""
    oi = PL.OracleIndex(gen)
    try:
        return [[(oi.pairings_depths(e, L, rate) if depths else oi.pairings(e, L, rate)) for e in ests] for L, rate in params]
    finally:
        oi.close()


def reference_answers(jobs):
    """The reference's build_vertex_set (PL.RefIndex built at each min_factor_len asked for) on jobs = [(genomic, ests,
    params), ...], in a child process: its object code dies on some tiny genomes.  Answers as nested lists, shaped as
    oracle_answers, or None when the child died."""
    req = json.dumps([[g.decode("latin-1"), [e.decode("latin-1") for e in ests], [list(p) for p in params]]
                      for g, ests, params in jobs])
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], input=req, capture_output=True, text=True)
    return json.loads(r.stdout) if r.returncode == 0 else None


def _reference_child():
    out = []
    for g, ests, params in json.load(sys.stdin):
        gen, ri, per_param = g.encode("latin-1"), {}, []
        for L, rate in params:
            if L not in ri:
                ri[L] = PL.RefIndex(gen, L)
            per_param.append([ri[L].pairings(e.encode("latin-1"), L, rate).tolist() if e else [] for e in ests])
        out.append(per_param)
    json.dump(out, sys.stdout)


def occurrences(gen, est, i, L):
    """Unfiltered: (t, l) of every occurrence of est[i:i + L] in gen that is not prev-excluded, l = the length of its match
    with est[i:] (plain Python; the copies of t == 0 count once)."""
    q, out = est[i:i + L], []
    if len(q) < L:
        return out
    t = gen.find(q)
    while t >= 0:
        if not (i > 0 and t > 0 and gen[t - 1] == est[i - 1]):
            l = L
            while i + l < len(est) and t + l < len(gen) and est[i + l] == gen[t + l]:
                l += 1
            out.append((t, l))
        t = gen.find(q, t + 1)
    return out


def double_threshold(D, rate, L):
    return int(max(float(D) * rate, float(L)))                               # src/max-emb-graph.c:273-274


def exact_threshold(D, rate, L):
    return max(D * Fraction(str(rate)), Fraction(L)).__floor__()


# ---- tags: what a case reached ----------------------------------------------------------------------------------------
# tags(group, case, answers) -> set; answers = oracle_answers(..., depths=True)

def _triples(tri):
    return {tuple(int(v) for v in r) for r in tri}


def _planted_offsets(name):
    f = dict((p[0], p[1:]) for p in name.split("/") if p[:1] in "ti" and p[1:].isdigit())
    return int(f["t"]), int(f["i"])


def tags(group, case, answers):
    name, gen, ests, params = case
    out = set()
    if group == "small_L":
        for (L, rate), per_est in zip(params, answers):
            if any(len(tri) for tri, _ in per_est):
                out.add(("L", L))
            if any(len(e) >= L and e[:L] not in gen for e in ests):
                out.add(("absent", L))
    elif group == "windows":
        parts = name.split("/")
        ln = int(parts[-1][3:])
        kind = parts[1] if parts[1] in ("gend", "eend", "start") else "base"
        for k, (tri, _) in enumerate(answers[0]):
            for p, t, l in _triples(tri):
                if l == ln and gen[t:t + l] == ests[k][p:p + l]:
                    last_pat = k == len(ests) - 1
                    if kind == "base":
                        out.add(("res", t % 32, p % 32, ln))
                    elif kind == "gend" and t + l == len(gen):
                        out.add(("gend", ln, "past" if p + l < len(ests[k]) else "ends"))
                    elif kind == "eend" and p + l == len(ests[k]):
                        out.add(("eend", ln, "last" if last_pat else "behind"))
                    elif kind == "start" and t == 0:
                        out.add(("start", ln, p))
    elif group == "flagged":
        parts = name.split("/")
        if parts[1] in ("gen", "est", "both"):
            mode, byte, ln = parts[1], int(parts[2]), int(parts[4][3:])
            t, i = _planted_offsets(name)
            o = ln - 1 if parts[3] == "olast" else int(parts[3][1:])
            tri = _triples(answers[0][0][0])
            through = (i, t, ln) in tri
            covering = [1 for p, tt, l in tri if tt - p == t - i and p <= i + o < p + l]
            if mode == "both" and through:
                out.add(("both", byte))
            if mode != "both" and not covering:
                out.add((mode, byte))
                if byte == ord("a"):
                    out.add(("case", mode))
        elif parts[1] == "head":
            for per_est in answers:
                if all(len(tri) for tri, _ in per_est):
                    out.add(("head", int(parts[2])))
        else:
            if any(len(tri) for per_est in answers for tri, _ in per_est):
                out.add(("stretch", parts[2]))
    elif group == "order":
        for per_est in answers:
            for tri, _ in per_est:
                rows = [tuple(r) for r in tri.tolist()]
                if any(t == 0 and rows.count((p, t, l)) > 1 for p, t, l in set(rows)):
                    out.add("repeated")
        out.add(("sigma", len(set(gen))))
    elif group == "threshold":
        (L, rate), = params
        for tri, depth in answers[0]:
            for p, t, l in tri.tolist():
                if l < exact_threshold(int(depth[p]), rate, L):
                    out.add("truncation")
    elif group == "crowded":
        (L, rate), = params
        for k, (tri, depth) in enumerate(answers[0]):
            rows = _triples(tri)
            for i in range(len(ests[k])):
                D = int(depth[i])
                if D < L:
                    continue
                thr = double_threshold(D, rate, L)
                occ = sorted(x for x in occurrences(gen, ests[k], i, L) if x[1] >= thr)
                if len(occ) >= 64:
                    out.add("list64")
                for j, (tj, lj) in enumerate(occ):                            # survives filter (a), yet is not in the answer
                    dead = any((tj > ti and tj + lj <= ti + li) or (tj == ti + 1 and lj == li) for ti, li in occ[:j])
                    if not dead and (i, tj, lj) not in rows:
                        out.add("filter_b")
    elif group == "batch":
        out.add(("patterns", len(ests)))
        out.update(("len", len(e)) for e in ests)
        if not ests[0] and not ests[-1] and any(not a and not b for a, b in zip(ests, ests[1:])):
            out.add("empties")
    return out


def cover(tagged, lone):
    """tagged = {group: [tag set of a case, ...]} of the cases the reference answered, lone = the same of the cases only the
    oracle answered -> (counts for the fixture's table, what the cover still lacks).  Only min_factor_len 1, where the
    reference answers nothing, is looked for among the lone cases."""
    n = {g: {} for g in GROUPS}
    for g in GROUPS:
        for ts in tagged.get(g, []):
            for x in ts:
                n[g][x] = n[g].get(x, 0) + 1
    lone_L = {x[1] for ts in lone.get("small_L", []) for x in ts if x[0] == "L"}
    want = [("small_L", ("L", L)) for L in SMALL_LS if L not in REFERENCE_DIES_AT_L] + [("small_L", ("absent", L)) for L in SMALL_LS if L >= 7]
    want += [("windows", ("res", tr, ir, ln)) for tr in RES for ir in RES for ln in LENS]
    for ln in LENS:
        want += [("windows", ("gend", ln, "ends")), ("windows", ("gend", ln, "past")), ("windows", ("eend", ln, "last")),
                 ("windows", ("eend", ln, "behind")), ("windows", ("start", ln, 0))]
    for b in FLAG_BYTES:
        want += [("flagged", (m, b)) for m in ("gen", "est", "both", "head")]
    want += [("flagged", ("case", "gen")), ("flagged", ("case", "est")), ("flagged", ("stretch", "star")), ("flagged", ("stretch", "lower"))]
    want += [("crowded", "list64"), ("crowded", "filter_b"), ("batch", "empties")]
    want += [("batch", ("patterns", k)) for k in (63, 64, 65, 129)]
    want += [("batch", ("len", k)) for k in (0, 1, 14, 15, 63, 64, 65, 127, 128, 129, 2000)]
    lacks = ["%s: %r" % (g, x) for g, x in want if not n[g].get(x)]
    lacks += ["small_L: ('L', %d), by the oracle alone" % L for L in REFERENCE_DIES_AT_L if L not in lone_L]
    if n["threshold"].get("truncation", 0) < 3:
        lacks.append("threshold: fewer than 3 cases keep a pairing below the exact rational floor")
    if n["order"].get("repeated", 0) < 20:
        lacks.append("order: fewer than 20 cases hold a repeated (i, 0, l)")
    counts = {
        "small_L: values of L with a pairing": sum(1 for x in n["small_L"] if x[0] == "L"),
        "small_L: values of L with a pairing, answered by the oracle alone": len(lone_L & set(REFERENCE_DIES_AT_L)),
        "small_L: values of L with an EST whose first L-mer does not occur": sum(1 for x in n["small_L"] if x[0] == "absent"),
        "windows: (t mod 32, i mod 32, len) residues": sum(1 for x in n["windows"] if x[0] == "res"),
        "windows: lengths ending on the genome's last base, EST ending there / running on":
            "%d / %d" % tuple(sum(1 for x in n["windows"] if x[0] == "gend" and x[2] == w) for w in ("ends", "past")),
        "windows: lengths ending on the EST's last base, last pattern / patterns behind":
            "%d / %d" % tuple(sum(1 for x in n["windows"] if x[0] == "eend" and x[2] == w) for w in ("last", "behind")),
        "windows: lengths starting both sequences": sum(1 for x in n["windows"] if x[0] == "start" and x[2] == 0),
        "flagged: cases per byte (N n a * #), genome only": " ".join(str(n["flagged"].get(("gen", b), 0)) for b in FLAG_BYTES),
        "flagged: cases per byte, EST only": " ".join(str(n["flagged"].get(("est", b), 0)) for b in FLAG_BYTES),
        "flagged: cases per byte, both (match goes through)": " ".join(str(n["flagged"].get(("both", b), 0)) for b in FLAG_BYTES),
        "flagged: cases per byte, in the first 8 bases": " ".join(str(n["flagged"].get(("head", b), 0)) for b in FLAG_BYTES),
        "flagged: A against a (match stops), a in the genome / in the EST":
            "%d / %d" % (n["flagged"].get(("case", "gen"), 0), n["flagged"].get(("case", "est"), 0)),
        "order: cases with a repeated (i, 0, l)": n["order"].get("repeated", 0),
        "order: largest alphabet": max([x[1] for x in n["order"] if x != "repeated" and x[0] == "sigma"] or [0]),
        "threshold: cases keeping a pairing below the exact rational floor": n["threshold"].get("truncation", 0),
        "crowded: cases with a position of 64 or more candidates": n["crowded"].get("list64", 0),
        "crowded: cases where filter (b) removes a pairing": n["crowded"].get("filter_b", 0),
        "batch: plan sizes": " ".join(str(x[1]) for x in sorted(y for y in n["batch"] if y != "empties" and y[0] == "patterns")),
    }
    return counts, lacks


# ---- does the fixture notice what it is aimed at?  (the oracle alone) -------------------------------------------------

def _changed(gen, ests, params, stored):
    got = oracle_answers(gen, ests, params)
    return any(a.tolist() != b for pa, pb in zip(got, stored) for a, b in zip(pa, pb))


def notices(fixture):
    """fixture = {group: [(case, stored pairings as nested lists), ...]} -> the three counts of cases whose answer changes
    under a change of the inputs, or of the threshold rule, that the fixture is meant to tell apart"""
    upper = sum(_changed(c[1].upper(), [e.upper() for e in c[2]], c[3], st) for c, st in fixture["flagged"])
    masks = 0
    for g in GROUPS:
        for c, st in fixture[g]:
            if any(b"*" in e or b"#" in e for e in c[2]):
                masks += _changed(c[1], [e.replace(b"*", b"N").replace(b"#", b"N") for e in c[2]], c[3], st)
    exact = 0
    for c, _ in fixture["threshold"]:
        (L, rate), = c[3]
        hit = False
        for e, (_, depth) in zip(c[2], oracle_answers(c[1], c[2], c[3], depths=True)[0]):
            for i in range(len(e)):
                D = int(depth[i])
                if D >= L and double_threshold(D, rate, L) != exact_threshold(D, rate, L):
                    ls = [l for _, l in occurrences(c[1], e, i, L)]
                    hit |= sum(l >= double_threshold(D, rate, L) for l in ls) != sum(l >= exact_threshold(D, rate, L) for l in ls)
        exact += hit
    return {"flagged cases that change when both sequences are upper-cased": upper,
            "cases that change when * and # become N in the EST alone": masks,
            "threshold cases that change under the exact rational floor": exact}


def load_fixture(path):
    """{group: [(case, stored pairings, by), ...]} from tests/golden/pairing_edges.json.gz"""
    import gzip
    with gzip.open(path, "rt") as f:
        doc = json.load(f)
    out = {}
    for g in GROUPS:
        out[g] = [((c["name"], c["genomic"].encode("latin-1"), [e.encode("latin-1") for e in c["ests"]],
                    [tuple(p) for p in c["params"]]),
                   [[[flat[k:k + 3] for k in range(0, len(flat), 3)] for flat in per_est] for per_est in c["pairings"]], c["by"])
                  for c in doc["groups"][g]]
    return out


if __name__ == "__main__":
    _reference_child()
