"""CPU restatement of pgpu_index_gap_chains: FILTER 4 of get_EST_factorizations, check_gap_errors
(src/est-factorizations.c:1462-1545, called at :416-433), on one factorization.

gaps            the border loop, the verdict and the merging loop in Python over an `ops` object that answers the one
                device question (the border refinement of a gap): OracleOps asks tests/oracle_lib.py; the caps of the entry.
einval          the PGPU_EINVAL rules of the entry for one call.
make_world / make_case   generated factorizations: one to six exons planted in a seeded random sequence of about 60 kb
                with Ns and lower case sprinkled over it, EST gaps cut from the two ends of their introns or made of
                random bases, and an aim for each tag of the fixture's cover.  Only the aim `burset_tie` writes into the
                sequence, inside a zone at its start that no other case touches.
batch_arrays / expect_arrays   the arrays of the entry for a batch and for its answers.
device_route    today's route on the device: one plan of PGPU_DP_BORDERS jobs with PGPU_JOB_B_GENOMIC and tail 0, with
                the logic of gaps() on the host around it.
load_fixture    tests/golden/gap_chains.json.gz (tools/make_gaps_golden.py).
"""
import gzip
import json
import os

import numpy as np

import oracle_lib as O
import refine_lib as RL

FIXTURE = os.path.join(RL.ROOT, "tests", "golden", "gap_chains.json.gz")
OK, ERANGE, EINVAL = 0, -34, -22
MAX_EXONS = 64            # PGPU_GAPS_MAX_EXONS
MAX_EST_GAP = 64          # PGPU_GAPS_MAX_EST_GAP
MAX_ERRORS = 20           # PGPU_GAPS_MAX_ERRORS: threshold_ed of :1465
MERGED = 0x80
TAGS = ("merged", "merged_run", "short_window", "gap_equals_intron", "burset_tie", "total_20", "total_21", "gap_64", "no_gap",
        "single_exon", "lower_or_N")

# A, C, G, T of either case exchanged with letters getBursetFrequency does not know: equality between bytes is kept, every
# frequency becomes 0, and the cut scan of general_refine_borders takes the first cut with the smallest total
_BLIND = bytes.maketrans(b"ACGTacgtEFHIefhi", b"EFHIefhiACGTacgt")


class OracleOps:
    """the one question, answered by the CPU oracle: refine_borders(p, t, max_errs = len(p)) with nothing behind t"""

    def borders(self, p: bytes, t: bytes, gen_off: int):
        return O.refine_borders(p, t, 0, len(p), len(p))


ORACLE = OracleOps()


def gaps(est: bytes, gen: bytes, exons, ops=ORACLE, info=None):
    """One query -> (status, verdict, total, n_kept, exons afterwards, steps).  exons: [(EST_start, EST_end, GEN_start,
    GEN_end)], a query the entry accepts (einval); the exons afterwards and the steps are parallel to them.  `info` (a dict)
    receives what the fixture's cover counts."""
    tagged = info is not None                               # the tag burset_tie costs a second refinement per gap
    info = {} if info is None else info
    orig = [tuple(int(v) for v in e) for e in exons]
    n = len(orig)
    pairs = [(orig[i + 1][0] - orig[i][1] - 1, orig[i + 1][2] - orig[i][3] - 1) for i in range(n - 1)]
    if n > MAX_EXONS or any(gp > MAX_EST_GAP for gp, _ in pairs):
        info["refused"] = "more than %d exons" % MAX_EXONS if n > MAX_EXONS else "an EST gap longer than %d" % MAX_EST_GAP
        return ERANGE, 0, 0, 0, orig, [0] * n
    ex = [list(e) for e in orig]
    steps = [0] * n
    total = 0
    info["single_exon"] = n == 1
    info["no_gap"] = n >= 2 and all(gp == 0 for gp, _ in pairs)
    # ---- the border loop (:1475-1514): every gap's two strings are the input's
    for i, (gap_p, gap_t) in enumerate(pairs):
        assert 0 <= gap_p <= gap_t                          # einval: the order of the exons, the FATAL of :1485
        if gap_p == 0:
            continue
        d, a = orig[i], orig[i + 1]
        p, t = est[d[1] + 1:a[0]], gen[d[3] + 1:a[2]]
        assert len(p) == gap_p and len(t) == gap_t
        r = ops.borders(p, t, d[3] + 1)
        assert r["ok"] == 1 and r["ed"] <= gap_p            # the refusal of :1508 is dead: the total is at most len_p
        if tagged:
            blind = O.refine_borders(p.translate(_BLIND), t.translate(_BLIND), 0, gap_p, gap_p)
            assert blind["ed"] == r["ed"]
            if (blind["off_p"], blind["off_t1"], blind["off_t2"]) != (r["off_p"], r["off_t1"], r["off_t2"]):
                info["burset_tie"] = True
        if gap_t < 2 * gap_p:
            info["short_window"] = True
        if gap_t == gap_p:
            info["gap_equals_intron"] = True
        if gap_p == MAX_EST_GAP:
            info["gap_64"] = True
        if any(c not in b"ACGT" for c in p + t[:2 * gap_p] + t[max(0, gap_t - 2 * gap_p):]):
            info["lower_or_N"] = True
        total += r["ed"]
        ex[i][1] = d[1] + r["off_p"]                        # :1502-1506
        ex[i + 1][0] = ex[i][1] + 1
        ex[i][3] = d[3] + r["off_t1"]
        ex[i + 1][2] = a[2] - (gap_t - r["off_t2"])
        steps[i + 1] = 1 + r["ed"]
    info["total_20"], info["total_21"] = total == 20, total == 21
    if total > MAX_ERRORS:
        return OK, 1, total, 0, [tuple(e) for e in ex], steps
    # ---- the merging loop (:1522-1542)
    dn, kept = 0, 1
    for i in range(1, n):
        if ex[i][2] - ex[dn][3] - 1 <= 3:
            ex[dn][1], ex[dn][3] = ex[i][1], ex[i][3]
            steps[i] |= MERGED
            info["merged"] = True
            if steps[i - 1] & MERGED:
                info["merged_run"] = True
        else:
            dn = i
            kept += 1
    return OK, 0, total, kept, [tuple(e) for e in ex], steps


def tags_of(info):
    return sorted(t for t in TAGS if info.get(t))


# ---- the PGPU_EINVAL rules ------------------------------------------------------------------------------------------
def einval(ests_len, gen_len, exons, queries):
    """True when pgpu_index_gap_chains refuses the whole call.  exons: array or list of 4-tuples; queries: records or
    dicts with the fields of pgpu_gaps_query."""
    named = set()
    for q in queries:
        est_off, est_len, first, n = int(q["est_off"]), int(q["est_len"]), int(q["first_exon"]), int(q["n_exons"])
        if est_off > ests_len or est_len > ests_len - est_off or est_len == 0 or est_len > 0x7FFFFFFF or int(q["reserved"]) != 0:
            return True
        if n == 0 or first > len(exons) or n > len(exons) - first:
            return True
        mine = []
        for k in range(first, first + n):
            if k in named:
                return True
            named.add(k)
            es, ee, gs, ge = (int(v) for v in exons[k])
            if not (-1 <= es <= est_len and -1 <= ee <= est_len and -1 <= gs <= gen_len and -1 <= ge <= gen_len):
                return True
            mine.append((es, ee, gs, ge))
        for d, a in zip(mine, mine[1:]):
            if d[1] >= a[0] or d[3] >= a[2] or a[0] - d[1] - 1 > a[2] - d[3] - 1:
                return True
    return False


# ---- generated inputs -----------------------------------------------------------------------------------------------
GEN_LEN = 60_000
TIE_ZONE = 12_000         # the aim `burset_tie` writes into [0, TIE_ZONE); every other case lies behind it
AIMS = (None, None, None, "merged", "merged_run", "short_window", "gap_equals_intron", "burset_tie", "total_20", "total_21",
        "gap_64", "no_gap", "single_exon", "lower_or_N", "dropped", "dropped")
_ACGT = b"ACGT"


def make_sequence(seed, length=GEN_LEN):
    """seeded random bases; behind the tie zone a few Ns and runs of lower case"""
    rng = np.random.default_rng(seed)
    g = bytearray(RL.rnd(rng, length))
    for _ in range(length // 400):
        p = int(rng.integers(TIE_ZONE, length - 40))
        if rng.random() < 0.5:
            g[p] = 78 if rng.random() < 0.8 else 110
        else:
            k = int(rng.integers(1, 30))
            g[p:p + k] = bytes(g[p:p + k]).lower()
    return g


def _noisy(rng, s, rate):
    """substitutions, insertions and deletions at `rate` per base; never empty"""
    out = bytearray()
    for c in s:
        r = rng.random()
        if r < rate / 3:
            continue
        if r < 2 * rate / 3:
            out.append(_ACGT[int(rng.integers(4))])
        elif r < rate:
            out.append(_ACGT[int(rng.integers(4))])
            continue
        out.append(c)
    return bytes(out) if out else bytes(s[:1])


def _from_ends(rng, intron, gap_p, rate):
    """an EST gap of about gap_p bases: a prefix and a suffix of the intron, with errors"""
    k = int(rng.integers(0, gap_p + 1))
    piece = bytes(intron[:k]) + bytes(intron[len(intron) - (gap_p - k):] if gap_p > k else b"")
    return _noisy(rng, piece, rate)[:MAX_EST_GAP]


def _junction(rng, g, at, kind):
    """what lies between two exons: (the EST gap, the length of the genomic gap that begins at g[at])"""
    if kind == "plain":                                      # no EST gap, an intron
        return b"", int(rng.integers(40, 400))
    if kind == "close":                                      # no EST gap, 0 .. 5 genomic bytes: merged up to 3
        return b"", int(rng.integers(0, 6))
    if kind == "ends":                                       # a short gap from the intron's two ends
        gap_p = int(rng.integers(1, 25))
        gap_t = 2 * gap_p + int(rng.integers(0, 300))
        return _from_ends(rng, g[at:at + gap_t], gap_p, float(rng.choice([0.0, 0.0, 0.05, 0.15]))), gap_t
    if kind == "equal":                                      # gapT == gapP: the gap is the intron, with substitutions
        gap = int(rng.integers(1, 40))
        p = bytearray(g[at:at + gap])
        for _ in range(int(rng.integers(0, 3))):
            p[int(rng.integers(gap))] = _ACGT[int(rng.integers(4))]
        return bytes(p), gap
    if kind == "short":                                      # gapP < gapT < 2 gapP
        gap_p = int(rng.integers(3, 50))
        gap_t = gap_p + int(rng.integers(1, gap_p))
        return _from_ends(rng, g[at:at + gap_t], gap_p, 0.05)[:gap_t], gap_t
    if kind == "g64":
        gap_t = 64 + int(rng.integers(0, 300))
        p = _from_ends(rng, g[at:at + gap_t], 64, 0.02)
        p = (p + bytes(g[at + gap_t - 64:at + gap_t]))[:64] if len(p) < 64 else p
        return p, gap_t
    if kind == "random":                                     # bases that match nowhere in particular
        gap_p = int(rng.integers(8, 65))
        return RL.rnd(rng, gap_p), gap_p + int(rng.integers(0, 300))
    raise ValueError(kind)


def _exact_errors(rng, g, at, want):
    """an EST gap whose refinement costs `want` where chance allows: the intron's first bases with `want` substitutions
    four apart, then its last ten (the DP may find cheaper: the case's tag is what the restatement measures, the aim only
    steers)"""
    gap_t = 200 + int(rng.integers(0, 100))
    pre, suf = bytearray(g[at:at + 4 * want + 2]), bytes(g[at + gap_t - 10:at + gap_t])
    for k in range(2, len(pre), 4):
        pre[k] = _ACGT[(_ACGT.index(pre[k] & ~32) + 1 + int(rng.integers(3))) % 4] if (pre[k] & ~32) in _ACGT else 65
    return bytes(pre) + suf, gap_t


def make_case(rng, g: bytearray, aim=None, tie_pos=None):
    """plants a factorization -> (est, exons, the end of its last exon): one to six exons of 15 to 90 bases copied
    from the sequence (the entry never reads an exon's bases), junctions of the kinds of _junction, flanks on the EST.
    `g` is written to only under the aim `burset_tie`, at tie_pos inside the tie zone."""
    n = int(rng.integers(1, 7))
    if aim == "single_exon":
        n = 1
    elif aim in ("merged", "short_window", "gap_equals_intron", "gap_64", "lower_or_N", "no_gap") and n < 2:
        n = 2
    elif aim in ("merged_run", "dropped", "total_20", "total_21") and n < 3:
        n = 3 + int(rng.integers(0, 3))
    if aim == "burset_tie":
        n = 2
    kinds = [str(rng.choice(["plain", "plain", "plain", "close", "ends", "ends", "equal", "short", "random"])) for _ in range(n - 1)]
    if aim == "no_gap":
        kinds = [str(rng.choice(["plain", "close"])) for _ in kinds]
    if aim == "merged":
        kinds[int(rng.integers(n - 1))] = str(rng.choice(["close", "equal"]))
    if aim == "merged_run":
        k = int(rng.integers(n - 2))
        kinds[k], kinds[k + 1] = str(rng.choice(["close", "equal"])), str(rng.choice(["close", "equal"]))
    if aim == "short_window":
        kinds[int(rng.integers(n - 1))] = "short"
    if aim == "gap_equals_intron":
        kinds[int(rng.integers(n - 1))] = "equal"
    if aim == "gap_64":
        kinds[int(rng.integers(n - 1))] = "g64"
    if aim == "dropped":
        kinds[0] = kinds[1] = "random"
    if aim in ("total_20", "total_21"):
        kinds = ["plain"] * (n - 1)
        kinds[0], kinds[1] = "exact10", "exact10" if aim == "total_20" else "exact11"
    ln0 = 0
    if aim == "burset_tie":
        kinds = ["tie"]
        at = tie_pos
    else:
        at = int(rng.integers(TIE_ZONE, len(g) - 6 * 120 - 5 * 420))
        if aim == "lower_or_N":                              # an exon that ends one to three bytes in front of an N or lower case
            odd = [i for i in range(at, min(at + 3000, len(g) - 3000)) if g[i] not in _ACGT]
            if odd:
                kinds[0] = str(rng.choice(["ends", "short", "random"]))
                ln0 = int(rng.integers(15, 60))
                at = odd[int(rng.integers(len(odd)))] - ln0 - int(rng.integers(0, 3))
    est, exons = bytearray(), []
    if rng.random() < 0.3:
        est += RL.rnd(rng, int(rng.integers(1, 40)))
    for i in range(n):
        ln = int(rng.integers(15, 90))
        if i == 0 and ln0:
            ln = ln0
        exons.append((len(est), len(est) + ln - 1, at, at + ln - 1))
        est += g[at:at + ln]
        at += ln
        if i == n - 1:
            break
        kind = kinds[i]
        if kind == "tie":
            # two cuts of no error, two bytes apart, the later one between GT and AG: the frequency moves the cut
            lp, lt = int(rng.integers(6, 20)), int(rng.integers(60, 120))
            i1 = int(rng.integers(1, lp - 3))
            p = bytearray(RL.rnd(rng, lp))
            p[i1:i1 + 2] = b"AG"
            g[at:at + i1 + 2] = p[:i1 + 2]
            g[at + i1 + 2:at + i1 + 4] = b"GT"
            g[at + lt - lp + i1:at + lt] = p[i1:]
            gap, gap_t = bytes(p), lt
        elif kind.startswith("exact"):
            gap, gap_t = _exact_errors(rng, g, at, int(kind[5:]))
        else:
            gap, gap_t = _junction(rng, g, at, kind)
        assert len(gap) <= gap_t and len(gap) <= MAX_EST_GAP
        est += gap
        at += gap_t
    if rng.random() < 0.3:
        est += RL.rnd(rng, int(rng.integers(1, 40)))
    assert at < len(g)
    return bytes(est), exons, at


def make_world(seed, n_cases, g=None):
    """(the sequence, [(est, exons)]): n_cases generated factorizations, the aims in turn"""
    rng = np.random.default_rng(seed)
    g = make_sequence(seed) if g is None else bytearray(g)
    cases, tie_pos = [], 50
    for k in range(n_cases):
        aim = AIMS[k % len(AIMS)]
        if aim == "burset_tie" and tie_pos + 400 > TIE_ZONE:
            aim = None
        est, exons, end = make_case(rng, g, aim, tie_pos)
        if aim == "burset_tie":
            tie_pos = end + 10
        cases.append((est, exons))
    return bytes(g), cases


def batch_arrays(cases):
    """cases of (est, exons) -> (ests, exons array, queries array) in the layouts of the entry; equal ESTs are stored once"""
    from pintron_amd import capi
    n_ex = sum(len(c[1]) for c in cases)
    exons = np.zeros(n_ex, dtype=np.dtype(capi.FACTOR_DTYPE))
    q = np.zeros(len(cases), dtype=np.dtype(capi.GAPS_QUERY_DTYPE))
    ests, eat, eoff, k = [], {}, 0, 0
    for i, (est, ex) in enumerate(cases):
        if est not in eat:
            eat[est] = eoff
            ests.append(est)
            eoff += len(est)
        for e in ex:
            exons[k] = tuple(e)
            k += 1
        q[i] = (eat[est], len(est), k - len(ex), len(ex), 0)
    return b"".join(ests), exons, q


def expect_arrays(exons, answers):
    """answers of gaps() per query, in the order of the exons -> the three arrays of the entry"""
    from pintron_amd import capi
    out_exons = exons.copy()
    out_steps = np.zeros(len(exons), dtype=np.uint8)
    res = np.zeros(len(answers), dtype=np.dtype(capi.GAPS_RESULT_DTYPE))
    k = 0
    for i, (status, verdict, total, kept, ex2, steps) in enumerate(answers):
        res[i] = (status, verdict, total, kept)
        for e, s in zip(ex2, steps):
            out_exons[k] = tuple(e)
            out_steps[k] = s
            k += 1
    assert k == len(exons)
    return out_exons, out_steps, res


def load_fixture():
    """(genomic bytes, [case dicts: est, exons, verdict, total, n_kept, exons_after, steps, tags])"""
    doc = json.load(gzip.open(FIXTURE, "rt"))
    g = bytearray(RL.rnd(np.random.default_rng(doc["seed"]), doc["length"]))
    for pos, s in doc["edits"]:
        g[pos:pos + len(s)] = s.encode()
    cases = []
    for est, ex, verdict, total, kept, after, steps, tags in doc["cases"]:
        cases.append(dict(est=est.encode(), exons=[tuple(e) for e in ex], verdict=verdict, total=total, n_kept=kept,
                          exons_after=[tuple(e) for e in after], steps=list(steps), tags=set(tags)))
    return bytes(g), cases


# ---- today's device route ---------------------------------------------------------------------------------------------
class _Asked(Exception):
    pass


class _DeviceOps:
    """answers from the plan; before it has run, the questions are collected"""

    def __init__(self):
        self.want, self.got = {}, None

    def borders(self, p, t, gen_off):
        key = (p, gen_off, len(t))
        if self.got is None:
            self.want.setdefault(key, len(self.want))
            return dict(ok=1, off_p=0, off_t1=0, off_t2=len(t), ed=0)
        return self.got[key]


def device_route(ctx, idx, gen: bytes, cases, clock=None):
    """cases of (est, exons) -> the answers of gaps(), every gap asked of the device as one PGPU_DP_BORDERS job
    (PGPU_JOB_B_GENOMIC: t is read from the resident sequence; tail 0) of ONE plan, with the glue of gaps() on the host.
    `clock` (a dict) receives "library_s", the seconds inside the plan's entry points, and "jobs"."""
    import ctypes as C
    import time
    from pintron_amd import capi
    ops = _DeviceOps()
    for est, ex in cases:
        gaps(est, gen, ex, ops=ops)
    keys = sorted(ops.want, key=ops.want.get)
    jl = capi.JobList()
    for p, off, lt in keys:
        jl.add(capi.BORDERS, p, bytes(lt), p0=0, p1=len(p), p2=len(p), b_gen_off=off, tail=0)      # b: its length alone
    L = ctx.L
    jobs, arena = jl.arrays()
    n = len(jl.jobs)
    res = (capi.DpResult * max(n, 1))()
    h = C.c_void_p()
    t0 = time.perf_counter()
    rc = L.pgpu_dp_plan_create(ctx.h, idx.h, jobs, n, arena, len(arena), C.byref(h))
    inside = time.perf_counter() - t0
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
    ops.got = {}
    for key, r in zip(keys, res):
        o = capi.decode(capi.BORDERS, r, b"")
        assert o["status"] == 0, o
        ops.got[key] = o
    if clock is not None:
        clock["library_s"], clock["jobs"] = inside, n
    return [gaps(est, gen, ex, ops=ops) for est, ex in cases]
