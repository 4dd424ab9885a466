"""CPU restatement of the side stage (pgpu_unit_sides, pgpu_pairing_plan_run_sides; the rule: include/pintron_gpu.h): from
the MEG records of a unit's patterns to its entries of megs.txt and processed-megs.txt and its lines of meg-edges.txt.

sides            queries and units (numpy, UNIT_QUERY_DTYPE / UNIT_RESULT_DTYPE), one record per pattern, one header per unit
                 and one (original) sequence per pattern -> (results as a numpy array of SIDE_RESULT_DTYPE, megs, pmegs,
                 edges).  Four arguments break the rule on purpose (the comparison must notice): WRONG.
record           a well-formed MEG record from vertices and adjacency lists: header, CSR, and the two texts by the formats
                 of meg_emit_kernel (pgpu_meg.hip) restated -- meg_text(), edges_text().
hand_cases       hand-made units; batch() lays a list of them out as one call, with units, patterns and records in three
                 different orders; tags_of() says what a case reaches; stretches() the (kind, source mod 4, destination mod 4,
                 length) of every stretch the copy loop moves in a laid-out batch.
program_sides    the program's three side files of one run, and per_est() to cut them into the texts of each input EST.
"""
import os
import random
import re
import struct

import numpy as np

import cand_lib as KL
import unit_lib as UL

NONE, DONE, HOST = 0, 1, 2                               # PGPU_SIDE_*
MAX_UNIT_BYTES = 1 << 24
SEP = b"\n\n***********\n\n"
WRONG = ("sibling_left_out", "sibling_added", "pmegs_from_fwd", "pattern_order")
LENGTHS = list(range(10)) + [63, 64, 65, 255, 256, 257]
FILES = ("megs.txt", "processed-megs.txt", "meg-edges.txt")
FLAGGED = KL.TOO_COMPLEX | KL.UNAVAILABLE


# ---- records -----------------------------------------------------------------------------------------------------------
def meg_text(vertices, adj):
    """meg_write (src/io-meg.c:146-190) as meg_emit_kernel prints it"""
    return ("".join("(%d,%d,%d)\n" % tuple(v) for v in vertices) + "#adj#\n" +
            "".join("%d-%d\n" % (a, b) for a, targets in enumerate(adj) for b in targets)).encode()


def edges_text(vertices, adj):
    """add_intronic_edges_to_file (src/max-emb-graph.c:677-699) as meg_emit_kernel prints it: one line per edge between
    two inner vertices"""
    out = []
    for a, targets in enumerate(adj):
        p, t, l = vertices[a]
        if p in (KL.SOURCE_P, KL.SINK_P):
            continue
        for b in targets:
            px, tx, lx = vertices[b]
            if px == KL.SINK_P:
                continue
            v = (t + l, tx, p + l, px, tx - t - l, px - p - l, (tx - t) - (px - p), l, lx)
            out.append(" ".join("%d" % x for x in v) + (" intronic" if v[6] >= 50 else "") + "\n")
    return "".join(out).encode()


def record(vertices, adj, flags=0):
    """a well-formed record: the graph and the two texts it prints"""
    return KL.record(vertices, adj, flags, meg_text(vertices, adj), edges_text(vertices, adj))


def filled(meg, edges):
    """a record whose two texts are the given bytes (the stage copies what the lengths name, whatever it says), behind the
    graph part of the empty graph"""
    return KL.record([SOURCE, SINK], [[], []], 0, meg, edges)


SOURCE, SINK = (KL.SOURCE_P, KL.SOURCE_P, KL.MARK_LEN), (KL.SINK_P, KL.SINK_P, KL.MARK_LEN)


def texts_of(rec):
    """(flags, M, X) of a record, or None when its graph part, its lengths and its texts pass its end"""
    if len(rec) < 16:
        return None
    nv, ne, flags, _ = struct.unpack_from("<4I", rec, 0)
    if flags & FLAGGED:
        return flags, b"", b""
    graph = (16 + 12 * nv + 2 * (nv + 1) + ne + 3) & ~3
    if graph + 8 > len(rec):
        return None
    ml, xl = struct.unpack_from("<2I", rec, graph)
    if graph + 8 + ml + xl > len(rec):
        return None
    return flags, rec[graph + 8:graph + 8 + ml], rec[graph + 8 + ml:graph + 8 + ml + xl]


# ---- the rule ----------------------------------------------------------------------------------------------------------
def entry(header, seq, meg):
    return b">" + header + b"\n" + seq + b"\n" + meg


def unit_sides(verdict, strand, fwd, rev, header, records, seqs, wrong=None):
    """(megs(u), pmegs(u), edges(u)) of a settled unit, or None when the unit is not one the rule covers"""
    has_sibling = rev != UL.NO_SIBLING
    if strand > 1 or (strand == 1 and not has_sibling) or (verdict == UL.U_UNALIGNED and strand == 0 and has_sibling):
        return None
    named = [fwd] + ([rev] if strand == 1 else [])
    got = {}
    for x in named:
        if x >= len(records):
            return None
        got[x] = texts_of(records[x])
        if got[x] is None or got[x][0] & FLAGGED:
            return None
    in_megs = list(named)
    if wrong == "sibling_left_out" and strand == 1:
        in_megs = [rev] if verdict == UL.U_ALIGNED else [fwd]
    if wrong == "sibling_added" and verdict == UL.U_ALIGNED and strand == 0 and has_sibling:
        got[rev] = texts_of(records[rev])
        in_megs = [fwd, rev]
    megs = b"".join(SEP + entry(header, seqs[x], got[x][1]) for x in in_megs)
    if verdict != UL.U_ALIGNED:
        return megs, b"", b""
    d = rev if strand == 1 else fwd
    p = fwd if wrong == "pmegs_from_fwd" else d
    return megs, entry(header, seqs[p], got[p][1]), b">" + header + b"\n" + got[d][2]


def sides(q, units, records, headers, seqs, wrong=None):
    """-> (results as a numpy array of SIDE_RESULT_DTYPE, megs, pmegs, edges); wrong: None or one of WRONG"""
    from pintron_amd import capi
    assert wrong is None or wrong in WRONG
    out = np.zeros(len(units), dtype=np.dtype(capi.SIDE_RESULT_DTYPE))
    made = []
    for i in range(len(units)):
        v = int(units["verdict"][i])
        if v == UL.U_HOST:
            continue
        strand, fwd, rev = int(units["strand"][i]), int(q["fwd"][i]), int(q["rev"][i])
        assert int(units["pattern"][i]) == (rev if strand else fwd)
        t = unit_sides(v, strand, fwd, rev, headers[i], records, seqs, wrong)
        if t is None or max(len(x) for x in t) > MAX_UNIT_BYTES:
            out["verdict"][i] = HOST
            continue
        out["verdict"][i] = DONE
        made.append((int(units["pattern"][i]) if wrong == "pattern_order" else i, i, t))
    blobs, at = ([], [], []), [0, 0, 0]
    for _, i, t in sorted(made, key=lambda m: m[:2]):
        for k, name in enumerate(("megs", "pmegs", "edges")):
            out[name + "_first"][i], out[name + "_bytes"][i] = at[k], len(t[k])
            at[k] += len(t[k])
            blobs[k].append(t[k])
    return (out,) + tuple(b"".join(b) for b in blobs)


# ---- hand-made cases ---------------------------------------------------------------------------------------------------
_made = {}


def _seq(rng, n):
    return bytes(rng.choices(b"ACGTN", k=n))


def _filler(rng, n, alphabet=b"(0123456789,)-#adj\n"):
    return bytes(rng.choices(alphabet, k=n))


def path(pairings):
    """the graph of a path over the given (p, t, l): source, the pairings, sink"""
    v = [SOURCE] + list(pairings) + [SINK]
    return v, [[k + 1] for k in range(len(v) - 1)] + [[]]


def _pat(seq, rec, at=None):
    """one pattern of a case: its sequence, its record, and the residue mod 4 its sequence begins at (None: wherever)"""
    return dict(seq=seq, rec=rec, at=at)


def _case_stretches(c, at):
    """the stretches one DONE case moves, given the running offsets `at` = [megs, pmegs, edges, headers]: {(kind, source mod
    4, destination mod 4, length)}; a stretch of length 0 counts with source 0.  A sequence whose residue is open counts
    as unknown (None) and covers nothing."""
    seen = set()

    def move(kind, src, dst, n):
        if src is not None:
            seen.add((kind, src % 4 if n else 0, dst % 4, n))

    hl, h_src = len(c["header"]), at[3]
    named = [c["f"]] + ([c["r"]] if c["strand"] == 1 else [])

    def put(dst, p):
        flags, M, X = texts_of(p["rec"])
        move("H", h_src, dst + 1, hl)
        move("S", p["at"], dst + 2 + hl, len(p["seq"]))
        move("M", 0, dst + 3 + hl + len(p["seq"]), len(M))
        return dst + 3 + hl + len(p["seq"]) + len(M)
    dst = at[0]
    for p in named:
        dst = put(dst + 15, p)
    if c["verdict"] == UL.U_ALIGNED:
        d = named[-1]
        put(at[1], d)
        flags, M, X = texts_of(d["rec"])
        move("H", h_src, at[2] + 1, hl)
        move("X", len(M), at[2] + 2 + hl, len(X))
    return seen


def _advance(c, at):
    """the running offsets behind a DONE case"""
    hl = len(c["header"])
    named = [c["f"]] + ([c["r"]] if c["strand"] == 1 else [])
    e = [hl + 3 + len(p["seq"]) + len(texts_of(p["rec"])[1]) for p in named]
    out = [at[0] + sum(15 + x for x in e), at[1], at[2], at[3] + hl]
    if c["verdict"] == UL.U_ALIGNED:
        out[1] += e[-1]
        out[2] += hl + 2 + len(texts_of(named[-1]["rec"])[2])
    return out


def needed_stretches():
    """every (kind, source mod 4, destination mod 4, length) the copy loop has to be seen with: M begins at a multiple of 4
    by the record's format, so its source residue is 0 alone"""
    out = set()
    for kind in "HSMX":
        for n in LENGTHS:
            for s in (range(4) if n and kind != "M" else (0,)):
                for d in range(4):
                    out.add((kind, s, d, n))
    return out


def hand_cases():
    """[dict(name, header, verdict, strand, f, r)]: f and r are _pat()s, r None for a unit without a sibling; a HOST unit
    has patterns too.  In unit order; shared, do not modify."""
    if "cases" in _made:
        return _made["cases"]
    rng = random.Random(4242)
    out = []

    def add(name, verdict, strand, f, r=None, header=None):
        out.append(dict(name=name, header=(b"/gb=S%04d /n=%d" % (len(out), len(out))) if header is None else header,
                        verdict=verdict, strand=strand, f=f, r=r))

    def some(n_pairs=2, sl=90, at=None):
        p = [(10 + 40 * k, 1000 + 300 * k + rng.randrange(50), 30 + rng.randrange(5)) for k in range(n_pairs)]
        return _pat(_seq(rng, sl), record(*path(p)), at)
    # every row of the table, with and without a sibling where the row allows both
    add("aligned_fwd_no_sibling", UL.U_ALIGNED, 0, some())
    add("aligned_fwd_with_sibling", UL.U_ALIGNED, 0, some(), some(3))
    add("aligned_rev", UL.U_ALIGNED, 1, some(1), some(4))
    add("unaligned_no_sibling", UL.U_UNALIGNED, 0, some())
    add("unaligned_rev", UL.U_UNALIGNED, 1, some(), some(1))
    add("host_between", UL.U_HOST, 0, some(), some())
    add("done_neighbour", UL.U_ALIGNED, 1, some(), some())
    add("host_rev_between", UL.U_HOST, 1, some(), some())
    add("host_no_sibling", UL.U_HOST, 0, some())
    add("unaligned_fwd_with_sibling_is_not_covered", UL.U_UNALIGNED, 0, some(), some())
    # a HOST unit may name flagged records; nobody reads them
    add("host_over_flagged", UL.U_HOST, 0, _pat(_seq(rng, 40), KL.bare(KL.UNAVAILABLE)), _pat(_seq(rng, 40), record(*path([(1, 2, 30)]), flags=KL.TOO_COMPLEX)))
    # the empty graph's record (two vertices, no edge): an EST that shares nothing with the genomic sequence
    add("empty_graph_unaligned", UL.U_UNALIGNED, 1, _pat(_seq(rng, 70), record([SOURCE, SINK], [[], []])),
        _pat(_seq(rng, 70), record([SOURCE, SINK], [[], []])))
    add("empty_graph_no_sibling", UL.U_UNALIGNED, 0, _pat(_seq(rng, 33), record([SOURCE, SINK], [[], []])))
    # an empty X: a graph with no inner edge (source -> one pairing -> sink)
    add("empty_X", UL.U_ALIGNED, 0, _pat(_seq(rng, 50), record(*path([(3, 700, 44)]))))
    add("empty_X_rev", UL.U_ALIGNED, 1, some(), _pat(_seq(rng, 50), record(*path([(0, 0, 15)]))))
    # intronic and not, negative differences
    add("intronic_edges", UL.U_ALIGNED, 0, _pat(_seq(rng, 200), record(*path([(0, 100, 40), (40, 190, 40), (80, 229, 40), (100, 5000, 60)]))))
    # a record at the device's caps: 64 vertices, a list of 32
    inner = [(2 * k, 100000 + 5000 * k, 15 + k % 7) for k in range(62)]
    v = [SOURCE] + inner + [SINK]
    adj = [list(range(1, 33))] + [[min(k + 1 + j, 63) for j in range(1)] for k in range(1, 63)] + [[]]
    adj[1] = list(range(2, 34))
    add("at_the_caps", UL.U_ALIGNED, 1, some(), _pat(_seq(rng, 400), record(v, adj)))
    # X's source residue steered by meg_text_len, through the digits of p, t, l
    for digits in range(4):
        g = path([(1, 10 ** digits, 20), (30, 10 ** digits + 2000, 21)])
        add("x_residue_by_digits_%d" % digits, UL.U_ALIGNED, digits & 1, _pat(_seq(rng, 64 + digits), record(*g)),
            _pat(_seq(rng, 61), record(*g)) if digits & 1 else None)
    # headers of 0-7 bytes, of odd bytes; sequences of 0 and 1 bases
    for hl in range(8):
        add("header_%d" % hl, (UL.U_ALIGNED, UL.U_UNALIGNED)[hl & 1], 1, some(), some(), header=b"hdr4567"[:hl])
    add("header_of_odd_bytes", UL.U_ALIGNED, 0, some(), header=bytes([0, 255, 10, 62, 35, 0, 128]) + b"tail")
    add("sequence_of_0", UL.U_ALIGNED, 1, _pat(b"", record(*path([(0, 5, 1)]))), _pat(b"", record(*path([(0, 7, 1), (1, 900, 1)]))))
    add("sequence_of_1", UL.U_ALIGNED, 1, _pat(b"G", record(*path([(0, 5, 1)]))), _pat(b"C", record(*path([(0, 6, 1)]))))
    add("sequence_of_0_unaligned", UL.U_UNALIGNED, 0, _pat(b"", record([SOURCE, SINK], [[], []])), header=b"")
    # every source residue, destination residue and length of every kind of stretch: the cases that follow are chosen, one
    # after the other, among seeded candidates for the most combinations not seen yet, given where the batch stands
    at, seen = [0, 0, 0, 0], set()
    for c in out:
        if _done(c):
            seen |= _case_stretches(c, at)
            at = _advance(c, at)
        else:
            at[3] += len(c["header"])
    need = needed_stretches()
    k = 0
    while need - seen:
        # the first combination still missing is aimed at -- its length and its source residue are set, the rest is drawn --;
        # a header's source residue is where the headers before it end, so a HOST unit with a header of 0-3 bytes may go first
        kind, s, d, n = min(need - seen)
        best, gain = None, 0
        for _ in range(64):
            pick = lambda w: n if w == kind else rng.choice(LENGTHS)
            gap = (s - at[3]) % 4 if kind == "H" else rng.choice((0, 0, 0, 1, 2, 3))
            lead = [dict(name="sweep_%d_gap" % k, header=b"gap"[:gap], verdict=UL.U_HOST, strand=0,
                         f=_pat(b"", KL.bare(KL.UNAVAILABLE)), r=None)] if gap else []
            here = [at[0], at[1], at[2], at[3] + gap]
            ml = pick("M")
            if kind == "X":
                ml = rng.choice([v for v in LENGTHS if v % 4 == s])
            f = _pat(_seq(rng, rng.choice(LENGTHS)), filled(_filler(rng, rng.choice(LENGTHS)), _filler(rng, rng.choice(LENGTHS))), rng.randrange(4))
            r = _pat(_seq(rng, pick("S")), filled(_filler(rng, ml), _filler(rng, pick("X"), b"0123456789 -intronic\n")),
                     s if kind == "S" else rng.randrange(4))
            strand = rng.randrange(2)
            c = dict(name="sweep_%d" % k, header=_filler(rng, pick("H"), b"/gb=ABC123 xyz>"), verdict=UL.U_ALIGNED,
                     strand=strand, f=r if strand == 0 else f, r=r if strand == 1 else None)
            g = len(_case_stretches(c, here) - seen & need)
            if g > gain and (kind, s, d, n) in _case_stretches(c, here):
                best, gain, best_at = lead + [c], g, here
        assert best is not None, (kind, s, d, n)
        out += best
        seen |= _case_stretches(best[-1], best_at)
        at = _advance(best[-1], best_at)
        k += 1
    _made["cases"] = out
    return out


def _done(c):
    return c["verdict"] != UL.U_HOST and not (c["verdict"] == UL.U_UNALIGNED and c["strand"] == 0 and c["r"] is not None)


def cap_cases():
    """the cap on a unit's bytes: megs(u) of exactly 2^24 bytes on an UNALIGNED unit with a sibling (two sequences; the header
    tunes the count) is DONE, a byte more is HOST; pmegs(u) over the cap is HOST (megs(u) holds pmegs(u) and 15 bytes more,
    so the cap on pmegs never decides alone: pmegs of exactly 2^24 bytes is HOST by its megs, and megs of exactly 2^24 on an
    ALIGNED unit is DONE with a pmegs 15 bytes shorter); with DONE neighbours"""
    if "cap" in _made:
        return _made["cap"]
    rng = random.Random(99)
    small = lambda: _pat(_seq(rng, 80), record(*path([(1, 500, 30), (40, 900, 30)])))
    g = record(*path([(0, 100, 20)]))
    ml = len(texts_of(g)[1])
    # megs = 2 * (15 + hl + 3 + ml) + sl_f + sl_r
    hl = 40
    sl = MAX_UNIT_BYTES - 2 * (15 + hl + 3 + ml)
    a, b = _seq(rng, sl // 2), _seq(rng, sl - sl // 2)
    # pmegs = hl + 3 + ml + sl: exactly the cap, and megs 15 past it; a byte less leaves pmegs under and megs over
    one = _seq(rng, MAX_UNIT_BYTES - (3 + 3 + ml))
    out = [dict(name="cap_neighbour_1", header=b"n1", verdict=UL.U_ALIGNED, strand=0, f=small(), r=None),
           dict(name="cap_exact", header=b"h" * hl, verdict=UL.U_UNALIGNED, strand=1, f=_pat(a, g), r=_pat(b, g)),
           dict(name="cap_one_over", header=b"h" * hl, verdict=UL.U_UNALIGNED, strand=1, f=_pat(a, g), r=_pat(b + b"A", g)),
           dict(name="cap_neighbour_2", header=b"n2", verdict=UL.U_ALIGNED, strand=1, f=small(), r=small()),
           dict(name="cap_pmegs_exact_megs_over", header=b"abc", verdict=UL.U_ALIGNED, strand=0, f=_pat(one, g), r=None),
           dict(name="cap_megs_exact", header=b"abc", verdict=UL.U_ALIGNED, strand=0, f=_pat(one[:-15], g), r=None),
           dict(name="cap_pmegs_alone", header=b"abc", verdict=UL.U_ALIGNED, strand=1, f=_pat(b"", g), r=_pat(one + b"C", g)),
           dict(name="cap_neighbour_3", header=b"n3", verdict=UL.U_UNALIGNED, strand=0, f=small(), r=None)]
    _made["cap"] = out
    return out


def batch(cases, seed=3, shuffle=True):
    """cases -> (q, units, records, headers, seqs) as the entries take them: the patterns in a seeded order of their own --
    a pattern no unit names stands in front of a sequence that has to begin at a residue --, so that units and patterns
    are in different orders; the records follow the patterns, and rec_first is whatever their sizes give"""
    from pintron_amd import capi
    pats = []
    for i, c in enumerate(cases):
        pats.append((i, "f"))
        if c["r"] is not None:
            pats.append((i, "r"))
    if shuffle:
        random.Random(seed).shuffle(pats)
    seqs, records, index, at = [], [], {}, 0
    for i, w in pats:
        p = cases[i][w]
        if p["at"] is not None and at % 4 != p["at"]:
            gap = (p["at"] - at) % 4
            seqs.append(b"x" * gap)
            records.append(KL.bare(KL.UNAVAILABLE))                  # a pattern no unit names
            at += gap
        index[(i, w)] = len(seqs)
        seqs.append(p["seq"])
        records.append(p["rec"])
        at += len(p["seq"])
    n = len(cases)
    q = np.zeros(n, dtype=np.dtype(capi.UNIT_QUERY_DTYPE))
    units = np.zeros(n, dtype=np.dtype(capi.UNIT_RESULT_DTYPE))
    for i, c in enumerate(cases):
        fwd, rev = index[(i, "f")], index.get((i, "r"), UL.NO_SIBLING)
        q[i] = (1000 + i, fwd, rev, 0)
        units[i] = (c["verdict"], c["strand"], 0, 0, rev if c["strand"] else fwd, 0, 0, 0)
    return q, units, records, [c["header"] for c in cases], seqs


def stretches(q, units, records, headers, seqs, want):
    """{(kind, source mod 4, destination mod 4, length)} of every stretch of the DONE units of a laid-out batch, as the form
    without a plan places them (every array at a multiple of 256, headers and sequences one behind the other, every record
    at a multiple of 4)"""
    seq_at = np.concatenate([[0], np.cumsum([len(s) for s in seqs])])
    hdr_at = np.concatenate([[0], np.cumsum([len(h) for h in headers])])
    seen = set()
    for i in range(len(units)):
        if int(want["verdict"][i]) != DONE:
            continue
        fwd, rev, strand = int(q["fwd"][i]), int(q["rev"][i]), int(units["strand"][i])
        c = dict(header=headers[i], verdict=int(units["verdict"][i]), strand=strand,
                 f=_pat(seqs[fwd], records[fwd], int(seq_at[fwd])), r=_pat(seqs[rev], records[rev], int(seq_at[rev])) if strand else None)
        seen |= _case_stretches(c, [int(want["megs_first"][i]), int(want["pmegs_first"][i]), int(want["edges_first"][i]), int(hdr_at[i])])
    return seen


TAGS = ["aligned_fwd", "aligned_fwd_with_sibling", "aligned_rev", "unaligned_no_sibling", "unaligned_rev", "host", "not_covered",
        "empty_graph", "empty_X", "at_the_caps", "intronic", "not_intronic", "sequence_of_0", "sequence_of_1", "empty_header",
        "x_residue_0", "x_residue_1", "x_residue_2", "x_residue_3"]


def tags_of(c):
    """what one case reaches"""
    if c["verdict"] == UL.U_HOST:
        return {"host"}
    if not _done(c):
        return {"not_covered"}
    t = set()
    if c["verdict"] == UL.U_ALIGNED:
        t.add("aligned_rev" if c["strand"] else "aligned_fwd_with_sibling" if c["r"] is not None else "aligned_fwd")
    else:
        t.add("unaligned_rev" if c["strand"] else "unaligned_no_sibling")
    named = [c["f"]] + ([c["r"]] if c["strand"] == 1 else [])
    for p in named:
        if len(p["seq"]) in (0, 1):
            t.add("sequence_of_%d" % len(p["seq"]))
        nv, ne = struct.unpack_from("<2I", p["rec"], 0)
        flags, M, X = texts_of(p["rec"])
        if nv == 2 and ne == 0 and M == meg_text([SOURCE, SINK], [[], []]):
            t.add("empty_graph")
        if nv == 64 and M == meg_text(*_graph(p["rec"])) and max(len(a) for a in _graph(p["rec"])[1]) == 32:
            t.add("at_the_caps")
    if not c["header"]:
        t.add("empty_header")
    if c["verdict"] == UL.U_ALIGNED:
        flags, M, X = texts_of(named[-1]["rec"])
        if M == meg_text(*_graph(named[-1]["rec"])):              # a well-formed record
            t.add("x_residue_%d" % (len(M) % 4))
            if not X:
                t.add("empty_X")
            if b" intronic\n" in X:
                t.add("intronic")
            if re.search(rb"\d\n", X):
                t.add("not_intronic")
    return t


def _graph(rec):
    _, verts, adj = KL.parse(rec)
    return verts, adj


# ---- the program's own files -------------------------------------------------------------------------------------------
def program_sides(cwd):
    """(megs.txt, processed-megs.txt, meg-edges.txt) of a run in `cwd`"""
    out = []
    for name in FILES:
        with open(os.path.join(cwd, name), "rb") as f:
            out.append(f.read())
    return tuple(out)


def _cut_at_headers(text):
    """a file whose entries begin with a '>' line, cut into them"""
    parts = [p for p in re.split(rb"(?m)^(?=>)", text) if p]
    assert b"".join(parts) == text and all(p.startswith(b">") for p in parts)
    return parts


def _header_of(entry_text):
    assert entry_text.startswith(b">")
    return entry_text[1:entry_text.index(b"\n")]


def per_est(ids, megs, pmegs, edges):
    """{est_index: (its entries of megs.txt, its entry of processed-megs.txt, its lines of meg-edges.txt)} for the input
    ESTs whose headers are `ids`: megs.txt is cut at SEP, and consecutive entries with one header belong to one EST;
    the other two are cut at their '>' lines.  Every EST has an entry of megs.txt; one without an entry in the other two
    has b"" there.  The cut files join to the whole again."""
    assert len(set(ids)) == len(ids)
    where = {h: k for k, h in enumerate(ids)}
    parts = megs.split(SEP)
    assert parts[0] == b"" and b"".join(SEP + p for p in parts[1:]) == megs
    m = {}
    last = None
    for p in parts[1:]:
        h = _header_of(p)
        if h != last:
            assert where[h] not in m and (last is None or where[h] > where[last])      # in input order, once
            m[where[h]] = b""
            last = h
        m[where[h]] += SEP + p
    assert b"".join(m[k] for k in sorted(m)) == megs
    other = []
    for text in (pmegs, edges):
        cut = {}
        for p in _cut_at_headers(text):
            assert where[_header_of(p)] not in cut
            cut[where[_header_of(p)]] = p
        assert list(cut) == sorted(cut) and b"".join(cut.values()) == text
        other.append(cut)
    return {k: (m[k], other[0].get(k, b""), other[1].get(k, b"")) for k in m}
