"""CPU restatement of the unit stage (pgpu_unit_records, pgpu_pairing_plan_run_units; the rule: include/pintron_gpu.h): from
the finals of the patterns to one verdict per input EST and the bytes of the group est-fact writes for an ALIGNED one.

pattern_verdict  a pattern's final result, its exons and its empty-graph bit -> (ALIGNED / NONE / HOST, reason)
units            the finals as the entries take them (numpy arrays: results, exons, empty-graph bytes) and the unit queries
                 -> (results as a numpy array of UNIT_RESULT_DTYPE, the blob).  Six arguments break the rule on purpose (the
                 cases must notice): WRONG.
read_blob        a blob of packed records -> [(offset, n_bytes, est_index, [(polya, polyad, [exons])])]
hand_cases       hand-made units; batch() lays a list of them out as one call, the patterns in another order than the
                 units; tags_of() says what a case reaches under given parameters.
real_units       the unit table, the working and original sequences, fixed_strand and the polyA-suffix flags of c2, test-AMBN
                 and test-issue-13, from the host's own preparation (tests/hostcheck/unit_prep_main.c over ef_load_ests).
empty_bits       the empty-graph byte of MEG records: an unflagged record with n_vertices == 2 and n_edges == 0.
"""
import os
import random
import struct
import subprocess
import tempfile

import numpy as np

import cand_lib as KL
import final_lib as FL

HERE = os.path.dirname(os.path.abspath(__file__))
HOST, EMPTY, DONE = FL.HOST, FL.EMPTY, FL.DONE
U_HOST, U_UNALIGNED, U_ALIGNED = 0, 1, 2                 # PGPU_UNIT_*; a pattern's NONE is numbered as UNALIGNED
NO_SIBLING = 0xffffffff
FWD_SUFF, REV_SUFF = 1, 2
UB_VERY_SMALL_EXON = 2                                   # _UB_VERY_SMALL_EXON_LENGTH_ (src/factorization-refinement.c:97)
MAX_EXONS = 128
WRONG = ("sibling_after_host", "small_bound_1", "small_bound_3", "other_strand_flag", "r_index_off", "unit_number", "pattern_order")


def pattern_verdict(r, exons, empty, small_bound=UB_VERY_SMALL_EXON):
    """r: one final result (outcome, stage, detail, first_exon, n_exons); exons: the call's exon array; empty: the pattern's
    empty-graph bit -> (verdict, reason)"""
    outcome = int(r["outcome"])
    if outcome == DONE:
        first, n = int(r["first_exon"]), int(r["n_exons"])
        for k in range(first, first + n):
            if int(exons["EST_end"][k]) + 1 - int(exons["EST_start"][k]) <= small_bound:
                return U_UNALIGNED, 1
        return U_ALIGNED, 0
    if outcome == EMPTY:
        return U_UNALIGNED, 0
    if outcome == HOST and int(r["stage"]) == 0 and int(r["detail"]) == KL.NOT_PATH and empty:
        return U_UNALIGNED, 2
    return U_HOST, 0


def group_bytes(est_index, r, exons, suffix, pref_N, retain, r_index_off=False):
    """the group ef_write_factorization_records writes for one factorization (pintron_amd/host/ef_estfact.c)"""
    n, first = int(r["n_exons"]), int(r["first_exon"])
    written = bool(retain) or n > 2 or (n == 2 and suffix)
    if not written:
        return struct.pack("<II", est_index, 0)
    l_index = 0 if retain else 1
    r_index = n + 1 if retain or suffix else n
    if r_index_off and not retain:
        r_index += 1
    keep = [k for k in range(n) if l_index < k + 1 < r_index]
    out = struct.pack("<IIBBH", est_index, 1, int(r["polyA"]) if retain else 0, int(r["polyadenil"]) if retain else 0, len(keep))
    for k in keep:
        e = exons[first + k]
        u = lambda v: v & 0xffffffff
        out += struct.pack("<4I", u(int(e["EST_start"]) + 1), u(int(e["EST_end"]) + 1), u(pref_N + int(e["GEN_start"]) + 1),
                           u(pref_N + int(e["GEN_end"]) + 1))
    return out


def units(res, exons, empty, q, pref_N=0, retain=1, wrong=None):
    """-> (results as a numpy array of UNIT_RESULT_DTYPE, blob); wrong: None or one of WRONG"""
    from pintron_amd import capi
    assert wrong is None or wrong in WRONG
    bound = {"small_bound_1": 1, "small_bound_3": 3}.get(wrong, UB_VERY_SMALL_EXON)
    out = np.zeros(len(q), dtype=np.dtype(capi.UNIT_RESULT_DTYPE))
    groups = []
    for i in range(len(q)):
        fwd, rev, flags = int(q["fwd"][i]), int(q["rev"][i]), int(q["flags"][i])
        strand, pat = 0, fwd
        v, reason = pattern_verdict(res[pat], exons, empty is not None and empty[pat], bound)
        if rev != NO_SIBLING and (v == U_UNALIGNED or (wrong == "sibling_after_host" and v == U_HOST)):
            strand, pat = 1, rev
            v, reason = pattern_verdict(res[pat], exons, empty is not None and empty[pat], bound)
        out[i] = (v, strand, reason, 0, pat, 0, 0, 0)
        if v == U_ALIGNED:
            suffix = (flags >> (1 - strand if wrong == "other_strand_flag" else strand)) & 1
            g = group_bytes(i if wrong == "unit_number" else int(q["est_index"][i]), res[pat], exons, suffix, pref_N, retain,
                            r_index_off=wrong == "r_index_off")
            out["n_factorizations"][i] = struct.unpack_from("<I", g, 4)[0]
            out["n_bytes"][i] = len(g)
            groups.append((pat if wrong == "pattern_order" else i, i, g))
    blob, at = b"", 0
    for _, i, g in sorted(groups):
        out["first_byte"][i] = at
        at += len(g)
        blob += g
    return out, blob


def read_blob(blob):
    """[(offset, n_bytes, est_index, [(polya, polyad, [(EST_start, EST_end, GEN_start, GEN_end)])])]: every group to the end"""
    out, pos = [], 0
    while pos < len(blob):
        at = pos
        est_index, n_fact = struct.unpack_from("<II", blob, pos)
        pos += 8
        facts = []
        for _ in range(n_fact):
            polya, polyad, n = struct.unpack_from("<BBH", blob, pos)
            pos += 4
            facts.append((polya, polyad, [struct.unpack_from("<4i", blob, pos + 16 * k) for k in range(n)]))
            pos += 16 * n
        out.append((at, pos - at, est_index, facts))
    assert pos == len(blob)
    return out


def groups_by_index(blob):
    """{est_index: the bytes of its group}"""
    out = {}
    for at, n, est_index, _ in read_blob(blob):
        assert est_index not in out
        out[est_index] = blob[at:at + n]
    return out


def empty_bits(records):
    """a byte per MEG record: 1 for an unflagged record with n_vertices == 2 and n_edges == 0"""
    return np.array([struct.unpack_from("<3I", r, 0) == (2, 0, 0) for r in records], dtype=np.uint8)


def query_array(qs):
    from pintron_amd import capi
    q = np.zeros(len(qs), dtype=np.dtype(capi.UNIT_QUERY_DTYPE))
    for i, x in enumerate(qs):
        q[i] = tuple(x)
    return q


# ---- hand-made cases ------------------------------------------------------------------------------------------------
def _exons(lens, est_at=0, gen_at=1000):
    """consecutive exons of the given EST lengths, introns of 100 bases between them"""
    out = []
    for n in lens:
        out.append((est_at, est_at + n - 1, gen_at, gen_at + n - 1))
        est_at += n
        gen_at += n + 100
    return out


def pat(outcome, stage=0, detail=0, lens=(), empty=0, polyA=0, polyadenil=0, exons=None):
    """one pattern: what its final result says, its exons (DONE only) and its empty-graph bit"""
    ex = (_exons(lens) if exons is None else exons) if outcome == DONE else []
    return dict(dict.fromkeys(FL.FIELDS, 0), outcome=outcome, stage=stage, detail=detail, polyA=polyA, polyadenil=polyadenil,
                exons=ex, steps=[0] * len(ex), empty=empty)


def aligned(lens=(40, 50, 60), **kw):
    return pat(DONE, 5, 0, lens, **kw)


SIBLINGS = dict(aligned=lambda: aligned((31, 32, 33, 34)), none=lambda: pat(EMPTY, 1, 3), host=lambda: pat(HOST, 3, 1),
                no=lambda: None)


def hand_cases():
    """[dict(name, fwd, rev (a pattern or None), flags, est_index)]; shared, do not modify"""
    if _hand:
        return _hand
    out = _hand

    def add(name, fwd, rev=None, flags=0, est_index=None):
        out.append(dict(name=name, fwd=fwd, rev=rev, flags=flags, est_index=1000 + 7 * len(out) if est_index is None else est_index))

    for s, make in SIBLINGS.items():
        add("aligned+" + s, aligned(), make())
        for stage in range(6):
            add("empty_%d+%s" % (stage, s), pat(EMPTY, stage, 1), make())
        add("small+" + s, aligned((40, 2, 60)), make())
        add("graph+" + s, pat(HOST, 0, KL.NOT_PATH, empty=1), make())
        add("host+" + s, pat(HOST, 2, 1), make())
    for stage in range(1, 6):
        for detail in (1, 2):
            add("host_%d_%d" % (stage, detail), pat(HOST, stage, detail), aligned())
    add("not_path_graph", pat(HOST, 0, KL.NOT_PATH, empty=0), aligned())
    add("flagged", pat(HOST, 0, KL.NONE, empty=0), aligned())
    add("bit_on_flagged", pat(HOST, 0, KL.NONE, empty=1), aligned())
    add("bit_on_done", aligned(empty=1), pat(EMPTY, 0, 2))
    add("bit_on_empty", pat(EMPTY, 2, 1, empty=1), aligned(empty=1))
    add("bit_on_host", pat(HOST, 1, 1, empty=1), aligned())
    add("bit_on_stage1_detail1", pat(HOST, 1, KL.NOT_PATH, empty=1), aligned())       # detail 1 at another stage: a cap
    add("graph_rev", pat(EMPTY, 0, 2), pat(HOST, 0, KL.NOT_PATH, empty=1))
    add("graph_both", pat(HOST, 0, KL.NOT_PATH, empty=1), pat(HOST, 0, KL.NOT_PATH, empty=1))
    for where in range(3):
        for n in (1, 2, 3):
            lens = [40, 50, 60]
            lens[where] = n
            add("exon_%d_at_%d" % (n, where), aligned(lens), aligned((35, 36)))
            add("rev_exon_%d_at_%d" % (n, where), pat(EMPTY, 4, 1), aligned(lens), flags=REV_SUFF)
    for n in (1, 2, 3, 4):
        for flags in range(4):
            lens = (40, 50, 60, 70)[:n]
            add("n%d_flags%d_fwd" % (n, flags), aligned(lens, polyA=1, polyadenil=1), aligned((33, 34, 35)), flags)
            add("n%d_flags%d_rev" % (n, flags), pat(EMPTY, 5, 2), aligned(lens, polyA=1), flags)
            add("n%d_flags%d_alone" % (n, flags & 1), aligned(lens, polyadenil=1), None, flags & 1)
    for a in (0, 1):
        for d in (0, 1):
            add("polyA%d_polyadenil%d" % (a, d), aligned(polyA=a, polyadenil=d))
    add("exons_128", aligned([3] * MAX_EXONS, polyA=1), None, FWD_SUFF)
    add("exons_128_rev", pat(EMPTY, 1, 1), aligned([4] * MAX_EXONS), 0)
    add("index_0", aligned(), None, 0, est_index=0)
    add("index_max", aligned((41, 42, 43, 44)), None, 0, est_index=0xffffffff)
    add("negative_coordinates", aligned(exons=[(-1, 5, -1, 8), (6, 40, 2000, 2034), (41, 90, 3000, 3049)]))
    add("coordinates_wrap", aligned(exons=[(0, 40, 0, 40), (41, 2147483646, 2147483000, 2147483647), (50, 90, 3000, 3049)]))
    return out


_hand = []


def batch(cases, seed=5, shuffle=True):
    """cases -> (res, exons, empty, q) as the entries take them: the patterns in a seeded order of their own, so that units,
    patterns and exons are in three different orders; the exons compact, in pattern order, as the final stage leaves them"""
    slots = []
    for i, c in enumerate(cases):
        slots.append((i, "fwd"))
        if c["rev"] is not None:
            slots.append((i, "rev"))
    if shuffle:
        random.Random(seed).shuffle(slots)
    where = {s: k for k, s in enumerate(slots)}
    pats = [cases[i][side] for i, side in slots]
    res, exons, _ = FL.expect_arrays(pats)
    empty = np.array([p["empty"] for p in pats], dtype=np.uint8)
    q = query_array([(c["est_index"], where[(i, "fwd")], where[(i, "rev")] if c["rev"] is not None else NO_SIBLING, c["flags"])
                     for i, c in enumerate(cases)])
    return res, exons, empty, q


TAGS = (["fwd_aligned+" + s for s in ("aligned", "none", "host")] +
        ["fwd_%s+%s" % (k, s) for k in ["empty_%d" % st for st in range(6)] + ["small", "graph"] for s in ("aligned", "none", "host", "no")] +
        ["fwd_host", "not_path_with_a_graph", "flagged", "bit_elsewhere"] +
        ["exon_%d_%s" % (n, w) for n in (1, 2, 3) for w in ("first", "middle", "last")] +
        ["externals_off_n%d_%s%d" % (n, w, f) for n in (1, 2, 3, 4) for w in ("deciding", "other") for f in (0, 1)] +
        ["flags_carried", "flags_zeroed", "pref_N_0", "pref_N_positive", "exons_128", "index_0", "index_max"])


def _kind(p, bound=UB_VERY_SMALL_EXON):
    if p is None:
        return "no"
    r = dict(p, first_exon=0, n_exons=len(p["exons"]))
    ex = np.array([tuple(e) for e in p["exons"]], dtype=np.dtype(FL_FACTOR())).reshape(-1)
    v, reason = pattern_verdict(r, ex, p["empty"], bound)
    if v == U_ALIGNED:
        return "aligned"
    if v == U_HOST:
        return "host"
    return {0: "empty_%d" % p["stage"], 1: "small", 2: "graph"}[reason]


def FL_FACTOR():
    from pintron_amd import capi
    return capi.FACTOR_DTYPE


def tags_of(c, pref_N, retain):
    """what one case reaches under the given parameters"""
    t = set()
    f, r = _kind(c["fwd"]), _kind(c["rev"])
    if f == "aligned" and r != "no":
        t.add("fwd_aligned+" + ("none" if r not in ("aligned", "host") else r))
    elif f == "host":
        t.add("fwd_host")
    elif f != "aligned":
        t.add("fwd_%s+%s" % (f, r if r in ("aligned", "host", "no") else "none"))
    for p in (c["fwd"], c["rev"]):
        if p is None:
            continue
        cell = (p["outcome"], p["stage"], p["detail"])
        if cell == (HOST, 0, KL.NOT_PATH) and not p["empty"]:
            t.add("not_path_with_a_graph")
        if cell == (HOST, 0, KL.NONE) and not p["empty"]:
            t.add("flagged")
        if p["empty"] and cell != (HOST, 0, KL.NOT_PATH):
            t.add("bit_elsewhere")
    decides = None if f == "host" else c["fwd"] if f == "aligned" else c["rev"] if r == "aligned" else None
    looked = [c["fwd"]] + ([c["rev"]] if f not in ("aligned", "host") and c["rev"] is not None else [])
    for p in looked:
        ex = p["exons"]
        for k, e in enumerate(ex):
            n = e[1] + 1 - e[0]
            if n in (1, 2, 3) and len(ex) >= 3:
                t.add("exon_%d_%s" % (n, "first" if k == 0 else "last" if k == len(ex) - 1 else "middle"))
    if decides is not None:
        strand = 0 if decides is c["fwd"] else 1
        n = len(decides["exons"])
        if not retain and n <= 4:
            t.add("externals_off_n%d_deciding%d" % (n, (c["flags"] >> strand) & 1))
            t.add("externals_off_n%d_other%d" % (n, (c["flags"] >> (1 - strand)) & 1))
        if decides["polyA"] and decides["polyadenil"]:
            t.add("flags_carried" if retain else "flags_zeroed")
        t.add("pref_N_positive" if pref_N > 0 else "pref_N_0")
        if n == MAX_EXONS:
            t.add("exons_128")
        if c["est_index"] in (0, 0xffffffff):
            t.add("index_0" if c["est_index"] == 0 else "index_max")
    return t


SETTINGS = [(0, 1), (0, 0), (1234, 1), (1 << 30, 0)]          # (pref_N_length, retain_externals)


# ---- the real inputs, as the host prepares them -------------------------------------------------------------------------
_real = {}


def prep_binary():
    """tests/hostcheck/unit_prep_main.c linked against libestfact_check.so, compiled once per process into a directory of its own"""
    if "exe" not in _real:
        hc = os.path.join(HERE, "hostcheck")
        subprocess.run(["make", "-s", "-C", hc, "libestfact_check.so"], check=True)
        d = _real["dir"] = tempfile.TemporaryDirectory()
        exe = os.path.join(d.name, "unit_prep")
        subprocess.run(["gcc", "-std=gnu99", "-O2", "-Wall", "-Wextra", "-o", exe, os.path.join(hc, "unit_prep_main.c"), "-L" + hc,
                        "-lestfact_check", "-Wl,-rpath," + hc, "-lm", "-pthread"], check=True)
        _real["exe"] = exe
    return _real["exe"]


def prepared(gfa, efa):
    """the host's preparation of one input -> dict(genomic, pref_N, units [(est_index, fwd, rev, flags)], working, original,
    fixed [per unit])"""
    with tempfile.TemporaryDirectory() as d:
        for name, text in (("genomic.txt", gfa), ("ests.txt", efa)):
            with open(os.path.join(d, name), "w") as f:
                f.write(text)
        r = subprocess.run([prep_binary()], cwd=d, check=True, capture_output=True)
    lines = r.stdout.split(b"\n")
    head = lines[0].split()
    assert head[0] == b"gen"
    out = dict(genomic=lines[1], pref_N=int(head[1]), units=[], working=[], original=[], fixed=[])
    k, pending = 2, None
    while k + 2 < len(lines) and lines[k].startswith(b"pat "):
        _, has_rev, fixed, suff = lines[k].split()
        p = len(out["working"])
        out["working"].append(lines[k + 1])
        out["original"].append(lines[k + 2])
        assert len(lines[k + 1]) == len(lines[k + 2])
        if pending is not None:                          # the sibling of the entry before
            est_index, fwd, _, flags = pending
            out["units"].append((est_index, fwd, p, flags | (REV_SUFF if int(suff) else 0)))
            assert not int(has_rev) and not int(fixed)
            pending = None
        else:
            unit = (len(out["units"]), p, NO_SIBLING, FWD_SUFF if int(suff) else 0)
            out["fixed"].append(bool(int(fixed)))
            if int(has_rev):
                assert not int(fixed)
                pending = unit
            else:
                out["units"].append(unit)
        k += 3
    assert pending is None and k == len(lines) - 1 and lines[k] == b""
    return out


def real_units(source):
    """prepared() of "c2", "ambn" or "issue13" (cand_lib.real_inputs); computed once, do not modify"""
    if source not in _real:
        gfa, efa = KL.real_inputs()[source]
        _real[source] = prepared(gfa, efa)
    return _real[source]


def finals(gfa, efa, U, use_originals=True, base=None):
    """final_lib.final of every prepared sequence of an input under the defaults, over the host's first-attempt graphs:
    (answers, the empty-graph bytes).  use_originals False: the working sequence stands in for the original (`base`: the
    answers with the originals, taken over where the two sequences are equal)."""
    import fact_lib as F
    import meg_lib as M
    import small_lib as SL
    recs, genomic = KL.host_records(gfa, efa, M.DEFAULTS)
    exp, _ = M.first_attempt_megs(gfa, efa, M.DEFAULTS)
    assert genomic == U["genomic"] and [e["seq"] for e in exp] == U["working"]
    ops = SL.OracleOps(genomic)
    answers = []
    for k, (rec, est, orig) in enumerate(zip(recs, U["working"], U["original"])):
        if not use_originals and base is not None and orig == est:
            answers.append(base[k])
            continue
        cand = KL.candidate(rec, genomic, 15, 40)
        answers.append(FL.final(cand[0], orig if use_originals else est, est, genomic, cand[3], F.DEFAULTS, ops=ops))
    return answers, empty_bits(recs)


def real_finals(source):
    """finals() of a real input with its real originals; computed once, do not modify"""
    key = ("finals", source)
    if key not in _real:
        gfa, efa = KL.real_inputs()[source]
        _real[key] = finals(gfa, efa, real_units(source))
    return _real[key]


def unit_queries(U):
    return query_array(U["units"])


def program_records(exe, gfa, efa, retain, cwd, env=None):
    """the packed records est-fact (the binary `exe`) writes for an input under PINTRON_RECORDS_FILE"""
    os.makedirs(cwd, exist_ok=True)
    for name, text in (("genomic.txt", gfa), ("ests.txt", efa)):
        with open(os.path.join(cwd, name), "w") as f:
            f.write(text)
    e = dict(os.environ, PINTRON_RECORDS_FILE="records.bin")
    e.update(env or {})
    subprocess.run([exe] + ([] if retain else ["--retain-externals", "false"]), cwd=cwd, env=e, check=True, stderr=subprocess.DEVNULL)
    with open(os.path.join(cwd, "records.bin"), "rb") as f:
        return f.read()


def against_the_program(out, blob, q, program_blob):
    """every ALIGNED unit's group equals the program's of that est_index, every UNALIGNED unit has none, and nothing but
    HOST units is left out -> (ALIGNED units compared, UNALIGNED units, [units that disagree])"""
    theirs = groups_by_index(program_blob)
    n_aligned = n_unaligned = 0
    wrong, settled = [], set()
    for i in range(len(q)):
        idx, v = int(q["est_index"][i]), int(out["verdict"][i])
        if v == U_ALIGNED:
            n_aligned += 1
            settled.add(idx)
            at, n = int(out["first_byte"][i]), int(out["n_bytes"][i])
            if theirs.get(idx) != blob[at:at + n]:
                wrong.append(i)
        elif v == U_UNALIGNED:
            n_unaligned += 1
            settled.add(idx)
            if idx in theirs:
                wrong.append(i)
    host = {int(q["est_index"][i]) for i in range(len(q)) if int(out["verdict"][i]) == U_HOST}
    assert set(theirs) - settled <= host, sorted(set(theirs) - settled - host)[:10]
    return n_aligned, n_unaligned, wrong
