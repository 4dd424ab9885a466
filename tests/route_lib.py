"""Where a DP job runs: the routing of the plan builder (pintron_amd/csrc/pgpu_api.hip: ROUTES[], classify,
form_groups, form_batch) restated in plain Python, and a hand-written probe set with at least three jobs in every
cell of it.  TEST INFRASTRUCTURE: the census tests compare Plan.groups() with expected_groups().

A CELL is a route in one execution form.  17 routes; gap_wave, lev_wave<ED>, lev_wave<KBAND> and borders_coop have
a second form (a launch of their own beside the batch launch), align_band has two ends (settled inside the band,
finished by the follow-up launch): 22 cells, CELLS below.  The form of a segment route's job follows from its row
class alone; borders_coop changes form as a whole with the longest cooperative BORDERS pattern of the PLAN; whether
a banded ALIGN is settled follows from its score, which no group reports -- the oracle's score says it."""
import random

import dp_cases as D

# ---- constants of the sources (tests/test_route_cpu.py reads them out of the .hip / .h text and compares) ----
COOP_W = 4                         # pgpu_dp_kernels.hip
DP_BATCH_MAX_LDS = 64 * 1024       # pgpu_internal.h
ALIGN_BAND_HALF = 31               # pgpu_internal.h
ROW_CLASS_STRIPS = 128             # pgpu_internal.h
MAX_ROWS_LEV, MAX_ROWS_GAP, MAX_GAP_SIDE, MAX_GAP_CELLS, MAX_COLS = 65536, 2048, 16000, 1 << 27, 1048576   # pintron_gpu.h
LCF_KEYS_PER_LAUNCH = 65535        # form_groups: grid.y of lcf_kernel
LCFW_MAX_CELLS, LCFW_MAX_SUM, LCFSA_MAX_L2 = 16384, 4096, 64      # classify

# place of a route in the batch launch
OUTSIDE, SEGMENT, ROLE = "outside", "segment", "role"
# ROUTES[] in its order (= the order of the groups of a plan): name, place, big_from (row class from which a segment
# route's jobs keep a launch of their own; 0: none do)
ROUTES = [
    ("lev_wave<ALIGN,strips>", OUTSIDE, 0),
    ("align_coop", ROLE, 0),
    ("lev_wave<ALIGN>", SEGMENT, 0),
    ("gap_slow", OUTSIDE, 0),
    ("gap_wave", SEGMENT, 8),
    ("lev_wave<ED>", SEGMENT, 32),
    ("lev_wave<KBAND>", SEGMENT, 32),
    ("lcf", OUTSIDE, 0),
    ("borders_slow", OUTSIDE, 0),
    ("borders_coop", ROLE, 0),
    ("lev_wave<BORDERS,R=1>", SEGMENT, 0),
    ("lev_wave<AFFIX,strips>", OUTSIDE, 0),
    ("affix_coop", ROLE, 0),
    ("lev_wave<AFFIX,R=1>", SEGMENT, 0),
    ("lcf_sa", SEGMENT, 0),
    ("lcf_small", SEGMENT, 0),
    ("align_band", SEGMENT, 0),
]
ROUTE_NAMES = [r[0] for r in ROUTES]
BATCH = "dp_batch"
TWO_FORM = ("gap_wave", "lev_wave<ED>", "lev_wave<KBAND>", "borders_coop")

CELLS = [
    "lev_wave<ALIGN,strips>/own", "align_coop/batch", "lev_wave<ALIGN>/batch", "gap_slow/own",
    "gap_wave/batch", "gap_wave/own", "lev_wave<ED>/batch", "lev_wave<ED>/own",
    "lev_wave<KBAND>/batch", "lev_wave<KBAND>/own", "lcf/own", "borders_slow/own",
    "borders_coop/batch", "borders_coop/own", "lev_wave<BORDERS,R=1>/batch", "lev_wave<AFFIX,strips>/own",
    "affix_coop/batch", "lev_wave<AFFIX,R=1>/batch", "lcf_sa/batch", "lcf_small/batch",
    "align_band/settled", "align_band/unsettled",
]
assert len(CELLS) == 22 and len(set(CELLS)) == 22


def row_class(rows):
    """smallest R in 1, 2, 4 .. 64 with 64 R >= rows; beyond 4096 rows: the strips"""
    if rows > 4096:
        return ROW_CLASS_STRIPS
    R = 1
    while 64 * R < rows:
        R <<= 1
    return R


def borders_coop_lds(rows):
    """dynamic LDS of the cooperative BORDERS sweep, in the batch launch and outside it (dp_batch_lds_bytes,
    launch_borders_coop): two hand-off areas and four row-minima arrays of rows + 1 words"""
    return (2 * (COOP_W - 1) * 128 + 4 * (rows + 1)) * 4


# the longest cooperative BORDERS pattern the batch launch holds: 768 + 4 (rows + 1) <= 16384 words
BORDERS_COOP_LAST_IN_BATCH = (DP_BATCH_MAX_LDS // 4 - 2 * (COOP_W - 1) * 128) // 4 - 1
assert BORDERS_COOP_LAST_IN_BATCH == 3903


def index_info_of(genomic):
    """what classify knows of the resident index: its length and the first character that is not upper-case ACGT"""
    fb = next((i for i, c in enumerate(genomic) if c not in b"ACGT"), len(genomic))
    return dict(n=len(genomic), first_bad=fb)


def route_of(case, index_info=None):
    """(route name, row class) of a case as classify decides it; None: the job is refused (ERANGE / EINVAL)."""
    la, lb, k = len(case.a), len(case.b), case.kind
    lev = lambda R: "strips" if R == ROW_CLASS_STRIPS else ("wave" if R == 1 else "coop")   # noqa: E731
    if k == D.ALIGN:
        if la > MAX_ROWS_LEV or lb > MAX_COLS:
            return None
        R = row_class(la)
        if 64 < la <= 4096 and abs(la - lb) <= ALIGN_BAND_HALF:
            return "align_band", R
        return {"strips": "lev_wave<ALIGN,strips>", "coop": "align_coop", "wave": "lev_wave<ALIGN>"}[lev(R)], R
    if k == D.GAP:
        if la > MAX_GAP_SIDE or lb > MAX_GAP_SIDE or (la + 1) * (lb + 1) > MAX_GAP_CELLS:
            return None
        return ("gap_slow", ROW_CLASS_STRIPS) if la > MAX_ROWS_GAP else ("gap_wave", row_class(la))
    if k in (D.ED, D.KBAND):
        if min(la, lb) > MAX_ROWS_LEV or max(la, lb) > MAX_COLS:
            return None
        return ("lev_wave<ED>" if k == D.ED else "lev_wave<KBAND>"), row_class(min(la, lb))
    if k == D.LCF:
        if lb > 65535 or la >= 1 << 28:
            return None
        if index_info is not None and getattr(case, "a_gen_off", None) == 0 and la <= index_info["first_bad"] \
                and lb <= LCFSA_MAX_L2:
            wild = sum(1 for c in case.b if c in b"Nn")
            if wild <= 1 and all(c in b"ACGTNn" for c in case.b):
                return "lcf_sa", 0
        if la * lb <= LCFW_MAX_CELLS and la + lb <= LCFW_MAX_SUM:
            return "lcf_small", 0
        return "lcf", 0
    if k == D.BORDERS:
        if la > MAX_ROWS_LEV or min(la + case.p2, lb) > MAX_COLS or case.p0 > case.p1 or case.p1 > la:
            return None
        R = row_class(la)
        return {"strips": "borders_slow", "coop": "borders_coop", "wave": "lev_wave<BORDERS,R=1>"}[lev(R)], R
    if k == D.AFFIX:
        if la > MAX_ROWS_LEV or lb > MAX_COLS:
            return None
        R = row_class(la)
        return {"strips": "lev_wave<AFFIX,strips>", "coop": "affix_coop", "wave": "lev_wave<AFFIX,R=1>"}[lev(R)], R
    raise ValueError(k)


def expected_groups(cases, index_info=None):
    """The census of a plan over `cases`: dict(groups=[(name, jobs with a launch of their own)] in the order of
    Plan.groups(), the batch launch's entry last when anything runs in it; classified={route: jobs};
    batched={route: jobs inside the batch launch}; dp_batch=their sum)."""
    rows = {}
    for c in cases:
        r = route_of(c, index_info)
        if r is not None:
            rows.setdefault(r[0], []).append((r[1], len(c.a)))
    groups, classified, batched = [], {}, {}
    for name, place, big_from in ROUTES:
        if name not in rows:
            continue
        n = len(rows[name])
        classified[name] = n
        if name == "lcf":                           # keyed: at most 65535 jobs per launch
            for first in range(0, n, LCF_KEYS_PER_LAUNCH):
                groups.append((name, min(LCF_KEYS_PER_LAUNCH, n - first)))
            own = n
        else:
            if place == OUTSIDE:
                own = n
            elif place == SEGMENT:
                own = sum(1 for R, _ in rows[name] if big_from and R >= big_from)
            elif name == "borders_coop":            # all or nothing, by the longest pattern of the plan
                own = n if borders_coop_lds(max(la for _, la in rows[name])) > DP_BATCH_MAX_LDS else 0
            else:
                own = 0
            groups.append((name, own))
        batched[name] = n - own
    total = sum(batched.values())
    if total:
        groups.append((BATCH, total))
    return dict(groups=groups, classified=classified, batched=batched, dp_batch=total)


def cell_of(case, index_info=None, score=None):
    """The cell of a case in a plan of its own.  align_band needs the oracle's score: the band settles a job
    exactly when the score is at most its half-width (a banded value is never below the true one, and an
    alignment of at most 31 errors never leaves the band)."""
    name, _ = route_of(case, index_info)
    if name == "align_band":
        return name + ("/settled" if score <= ALIGN_BAND_HALF else "/unsettled")
    return name + ("/batch" if expected_groups([case], index_info)["batched"][name] else "/own")


# ---------------------------------------------------------------------------------------------
# the probe set
# ---------------------------------------------------------------------------------------------
class GenCase(D.Case):
    """LCF whose first operand is the prefix [0, len(a)) of the resident genomic sequence"""
    a_gen_off = 0

    def add_to(self, jl):
        return jl.add(self.kind, self.a, self.b, self.p0, self.p1, self.p2, self.b_tail, a_gen_off=0)


class Probe:
    def __init__(self, cell, case, note=""):
        self.cell, self.case, self.note = cell, case, note

    def __repr__(self):
        return "Probe(%s, %r%s)" % (self.cell, self.case, ", " + self.note if self.note else "")


# the resident sequence of the probes: upper-case ACGT up to an N at 4500
_gen_rng = random.Random(20261)
PROBE_GENOMIC = D.rand_seq(_gen_rng, 4500) + b"N" + D.rand_seq(_gen_rng, 499)
PROBE_INDEX_INFO = index_info_of(PROBE_GENOMIC)
assert PROBE_INDEX_INFO == dict(n=5000, first_bad=4500)


def _seeded(make):
    """Every probe draws from a generator of its own, the helper's first argument, seeded by the helper's name and
    arguments: adding, removing or reordering probes leaves the operands of all the others as they were."""
    def seeded(*args, **kw):
        return make(random.Random(repr((make.__name__, args, sorted(kw.items())))), *args, **kw)
    return seeded


def _seq(rng, n):
    return D.rand_seq(rng, n)


def _near(rng, a, m, rate=0.03):
    """a string of exactly m characters that starts as a mutated copy of a"""
    b = D.mutate(rng, a, rate)
    return (b + _seq(rng, max(0, m - len(b))))[:m]


@_seeded
def _align(rng, la, lb, rate=0.03):
    a = _seq(rng, la)
    return D.Case(D.ALIGN, a, _near(rng, a, lb, rate))


@_seeded
def _subs(rng, n, k):
    """ALIGN of n characters against themselves with k substitutions, three characters apart"""
    a = _seq(rng, n)
    b = bytearray(a)
    for q in range(k):
        b[3 * q + 1] = b"CGTA"[b"ACGT".index(a[3 * q + 1])]
    return D.Case(D.ALIGN, a, bytes(b))


@_seeded
def _gap(rng, la, lb):
    """EST window of la characters against la + intron characters of the genomic sequence, cut to lb"""
    a = _seq(rng, la)
    cut = la // 2
    g = a[:cut] + b"GT" + _seq(rng, max(0, lb - la - 4)) + b"AG" + a[cut:]
    return D.Case(D.GAP, a, g[:lb] if lb < len(g) else g + _seq(rng, lb - len(g)))


@_seeded
def _ed(rng, la, lb):
    n = max(la, lb)
    a = _seq(rng, n)
    b = _near(rng, a, n, 0.04)
    return D.Case(D.ED, a[:la], b[:lb])


@_seeded
def _kband(rng, la, lb, ub):
    n = max(la, lb)
    a = _seq(rng, n)
    b = _near(rng, a, n, 0.04)
    return D.Case(D.KBAND, a[:la], b[:lb], p0=ub)


@_seeded
def _identity(rng, n):
    a = _seq(rng, n)
    return D.Case(D.ALIGN, a, a)


@_seeded
def _lcf(rng, la, lb, wild=0, gen=False):
    """a planted common factor of up to 12 characters; `wild` Ns in s2; gen: s1 = the resident prefix"""
    s1 = PROBE_GENOMIC[:la] if gen else _seq(rng, la)
    s2 = bytearray(_seq(rng, lb))
    k = min(12, la, lb)
    if k >= 3:
        p = rng.randint(0, min(la, PROBE_INDEX_INFO["first_bad"] if gen else la) - k)
        q = rng.randint(0, lb - k)
        s2[q:q + k] = s1[p:p + k]
    for w in range(wild):
        s2[(7 + 11 * w) % lb] = ord("N")
    return (GenCase if gen else D.Case)(D.LCF, s1, bytes(s2))


@_seeded
def _borders(rng, la, extra, p0, p1, errs, tail=b""):
    """t = the pattern, mutated, with an intron of `extra` characters at a cut"""
    p = _seq(rng, la)
    cut = rng.randint(0, la)
    t = D.mutate(rng, p[:cut], 0.03) + b"GT" + _seq(rng, extra) + b"AG" + D.mutate(rng, p[cut:], 0.03)
    return D.Case(D.BORDERS, p, t, p0=p0, p1=p1, p2=errs, b_tail=tail)


@_seeded
def _borders_short(rng, la, lt, p0, p1, errs, tail=b""):
    """a long pattern against a short window of lt characters"""
    p = _seq(rng, la)
    return D.Case(D.BORDERS, p, _near(rng, p[:lt], lt), p0=p0, p1=p1, p2=errs, b_tail=tail)


@_seeded
def _affix(rng, la, lb):
    a = _seq(rng, la)
    b = _near(rng, a, lb, 0.05)
    if b and a:
        b = bytes([a[0] ^ 6]) + b[1:]          # the caller only asks when the first characters differ
    return D.Case(D.AFFIX, a, b)


_LAST = BORDERS_COOP_LAST_IN_BATCH          # 3903 (checked above and, against the sources, in test_route_cpu.py)
_E = D.Case                                  # literal operands of dp_cases.edge_cases()

PROBES = [
    # ---- ALIGN: strips beyond 4096 rows; four waves above 64 rows; one wave; the band ----
    Probe("lev_wave<ALIGN,strips>/own", _align(4097, 37)),
    Probe("lev_wave<ALIGN,strips>/own", _align(4097, 1)),
    Probe("lev_wave<ALIGN,strips>/own", _align(4130, 24), "lengths apart by far more than the band"),
    Probe("align_coop/batch", _align(65, 97), "length difference 32: one past the band"),
    Probe("align_coop/batch", _align(97, 65), "length difference 32, the other way round"),
    Probe("align_coop/batch", _align(4096, 40), "last row count below the strips"),
    Probe("align_coop/batch", _align(130, 1)),
    Probe("lev_wave<ALIGN>/batch", _align(64, 64), "64 rows: the band starts at 65"),
    Probe("lev_wave<ALIGN>/batch", _align(64, 200)),
    Probe("lev_wave<ALIGN>/batch", _E(D.ALIGN, b"", b"")),
    Probe("lev_wave<ALIGN>/batch", _E(D.ALIGN, b"", b"ACGT")),
    Probe("lev_wave<ALIGN>/batch", _E(D.ALIGN, b"ACGTNNACGT", b"")),
    Probe("lev_wave<ALIGN>/batch", _E(D.ALIGN, b"A", b"N")),
    Probe("align_band/settled", _align(65, 96, 0.0), "length difference 31 = the score: the last the band settles"),
    Probe("align_band/settled", _align(96, 65, 0.0), "length difference 31, the other way round"),
    Probe("align_band/settled", _align(65, 65, 0.02)),
    Probe("align_band/settled", _align(4096, 4090, 0.002), "last row count of the band"),
    Probe("align_band/settled", _identity(300), "identity"),
    Probe("align_band/settled", _subs(100, 31), "score 31: the last the band settles"),
    Probe("align_band/unsettled", _subs(100, 32), "score 32: the first it leaves to the follow-up launch"),
    Probe("align_band/unsettled", D.Case(D.ALIGN, b"AC" * 33, b"GT" * 33), "66 rows, score 66"),
    Probe("align_band/unsettled", _align(65, 96, 0.25), "length difference 31 and mismatches: above 31"),
    Probe("align_band/unsettled", _align(400, 395, 0.2)),
    Probe("align_band/unsettled", _align(1000, 1031, 0.1)),
    # ---- GAP: the anti-diagonal kernel beyond 2048 rows; own launch from 257 rows (R >= 8) ----
    Probe("gap_slow/own", _gap(2049, 100)),
    Probe("gap_slow/own", _gap(2049, 2200)),
    Probe("gap_slow/own", _gap(2100, 90)),
    Probe("gap_wave/own", _gap(257, 330), "first row count of R = 8"),
    Probe("gap_wave/own", _gap(2048, 120), "last row count of the fast kernels"),
    Probe("gap_wave/own", _gap(513, 700)),
    Probe("gap_wave/batch", _gap(256, 330), "last row count of R = 4"),
    Probe("gap_wave/batch", _gap(255, 40)),
    Probe("gap_wave/batch", _gap(60, 300)),
    Probe("gap_wave/batch", _E(D.GAP, b"", b"")),
    Probe("gap_wave/batch", _E(D.GAP, b"A", b"ACGTACGTACGTACGTACGT")),
    Probe("gap_wave/batch", _E(D.GAP, b"ACGTNNACGT", b"")),
    # ---- ED, KBAND: the shorter string is on the rows; own launch from 1025 rows (R >= 32) ----
    Probe("lev_wave<ED>/own", _ed(1025, 1025), "first row count of R = 32"),
    Probe("lev_wave<ED>/own", _ed(1025, 1300)),
    Probe("lev_wave<ED>/own", _ed(1400, 1025), "the rows are the second operand"),
    Probe("lev_wave<ED>/own", _ed(4097, 4100), "strips"),
    Probe("lev_wave<ED>/batch", _ed(1024, 1024), "last row count of R = 16"),
    Probe("lev_wave<ED>/batch", _ed(1024, 1500)),
    Probe("lev_wave<ED>/batch", _ed(4097, 30), "4097 characters against 30: 30 rows"),
    Probe("lev_wave<ED>/batch", _E(D.ED, b"", b"")),
    Probe("lev_wave<ED>/batch", _E(D.ED, b"N", b"ACGTACGTACGTACGTACGT")),
    Probe("lev_wave<ED>/batch", _E(D.ED, b"AAAAAAAAAA", b"")),
    Probe("lev_wave<KBAND>/own", _kband(1025, 1025, 41), "first row count of R = 32"),
    Probe("lev_wave<KBAND>/own", _kband(1025, 1040, 20), "band on the lanes"),
    Probe("lev_wave<KBAND>/own", _kband(1300, 1025, 1300)),
    Probe("lev_wave<KBAND>/own", _kband(4097, 4100, 170), "strips"),
    Probe("lev_wave<KBAND>/batch", _kband(1024, 1024, 41), "last row count of R = 16"),
    Probe("lev_wave<KBAND>/batch", _kband(1024, 1030, 7)),
    Probe("lev_wave<KBAND>/batch", _kband(4097, 30, 4097)),
    Probe("lev_wave<KBAND>/batch", _E(D.KBAND, b"", b"", p0=0)),
    Probe("lev_wave<KBAND>/batch", _E(D.KBAND, b"ACGT", b"", p0=3)),
    Probe("lev_wave<KBAND>/batch", _E(D.KBAND, b"A", b"ACGTNNACGT", p0=50)),
    # ---- LCF: the matrix kernel; one wave for two short strings; the suffix array for a resident prefix ----
    Probe("lcf/own", _lcf(257, 64), "257 x 64 = 16448 cells"),
    Probe("lcf/own", _lcf(129, 128), "129 x 128 = 16512 cells"),
    Probe("lcf/own", _lcf(4093, 4), "16372 cells, but 4097 characters"),
    Probe("lcf/own", _lcf(4096, 1), "4097 characters"),
    Probe("lcf/own", _lcf(4400, 65, gen=True), "resident prefix, 65 EST characters"),
    Probe("lcf/own", _lcf(4400, 64, wild=2, gen=True), "resident prefix, two Ns"),
    Probe("lcf/own", _lcf(4501, 40, gen=True), "resident prefix that reaches the sequence's N"),
    Probe("lcf_small/batch", _lcf(256, 64), "256 x 64 = 16384 cells"),
    Probe("lcf_small/batch", _lcf(128, 128), "128 x 128 = 16384 cells"),
    Probe("lcf_small/batch", _lcf(4092, 4), "16368 cells, 4096 characters"),
    Probe("lcf_small/batch", _lcf(4095, 1), "4096 characters"),
    Probe("lcf_small/batch", _lcf(252, 65, gen=True), "resident prefix, 65 EST characters, 16380 cells"),
    Probe("lcf_small/batch", _lcf(200, 64, wild=2, gen=True), "resident prefix, two Ns"),
    Probe("lcf_small/batch", _E(D.LCF, b"", b"")),
    Probe("lcf_small/batch", _E(D.LCF, b"ACGTNNACGT", b"A")),
    Probe("lcf_small/batch", _E(D.LCF, b"", b"ACGTACGTACGTACGTACGT")),
    Probe("lcf_sa/batch", _lcf(4400, 64, gen=True), "64 EST characters"),
    Probe("lcf_sa/batch", _lcf(4400, 64, wild=1, gen=True), "one N"),
    Probe("lcf_sa/batch", _lcf(4500, 46, gen=True), "the prefix ends in front of the sequence's N"),
    Probe("lcf_sa/batch", _lcf(200, 30, wild=1, gen=True), "short enough for lcf_small, but resident"),
    Probe("lcf_sa/batch", _lcf(0, 20, gen=True), "empty prefix"),
    # ---- BORDERS: the anti-diagonal kernel beyond 4096 rows; eight waves above 64; one wave ----
    Probe("borders_slow/own", _borders_short(4097, 60, 0, 4097, 3)),
    Probe("borders_slow/own", _borders_short(4097, 45, 1300, 2700, 0, b"GT")),
    Probe("borders_slow/own", _borders_short(4100, 1, 0, 4100, 2, b"A")),
    Probe("borders_coop/batch", _borders(_LAST, 120, 0, _LAST, 40), "last row count the batch launch's LDS holds"),
    Probe("borders_coop/batch", _borders(_LAST - 1, 60, 1300, 2600, 3, b"GT")),
    Probe("borders_coop/batch", _borders(65, 150, 0, 65, 6, b"A"), "first row count above one wave"),
    Probe("borders_coop/batch", _borders_short(3000, 50, 0, 3000, 2)),
    Probe("borders_coop/own", _borders(_LAST + 1, 120, 0, _LAST + 1, 40), "first row count past the LDS"),
    Probe("borders_coop/own", _borders_short(_LAST + 2, 50, 1300, 2600, 3, b"GT")),
    Probe("borders_coop/own", _borders_short(4096, 70, 0, 4096, 0, b"A"), "last row count below the slow kernel"),
    Probe("lev_wave<BORDERS,R=1>/batch", _borders(64, 150, 0, 64, 6, b"GT"), "last row count of one wave"),
    Probe("lev_wave<BORDERS,R=1>/batch", _borders(30, 40, 10, 20, 3)),
    Probe("lev_wave<BORDERS,R=1>/batch", _E(D.BORDERS, b"", b"", p0=0, p1=0, p2=0)),
    Probe("lev_wave<BORDERS,R=1>/batch", _E(D.BORDERS, b"ACGT", b"", p0=2, p1=4, p2=2, b_tail=b"GT")),
    Probe("lev_wave<BORDERS,R=1>/batch", _E(D.BORDERS, b"", b"ACGTNNACGT", p0=0, p1=0, p2=30)),
    # ---- AFFIX ----
    Probe("lev_wave<AFFIX,strips>/own", _affix(4097, 37)),
    Probe("lev_wave<AFFIX,strips>/own", _affix(4097, 1)),
    Probe("lev_wave<AFFIX,strips>/own", _affix(4200, 64)),
    Probe("affix_coop/batch", _affix(65, 65), "first row count above one wave"),
    Probe("affix_coop/batch", _affix(4096, 50), "last row count below the strips"),
    Probe("affix_coop/batch", _affix(1025, 1)),
    Probe("lev_wave<AFFIX,R=1>/batch", _affix(64, 300), "last row count of one wave"),
    Probe("lev_wave<AFFIX,R=1>/batch", _E(D.AFFIX, b"", b"")),
    Probe("lev_wave<AFFIX,R=1>/batch", _E(D.AFFIX, b"A", b"")),
    Probe("lev_wave<AFFIX,R=1>/batch", _E(D.AFFIX, b"", b"ACGTACGTACGTACGTACGT")),
]


def oracle_cells(case):
    """matrix cells the CPU oracle fills for a case (BORDERS: two sweeps of len_p x t_win)"""
    la, lb = len(case.a), len(case.b)
    if case.kind == D.BORDERS:
        return 2 * (la + 1) * (min(la + case.p2, lb) + 1)
    return (la + 1) * (lb + 1)


def probes_of(cell):
    return [p for p in PROBES if p.cell == cell]


def probe_cases(cell=None):
    return [p.case for p in PROBES if cell is None or p.cell == cell]


def observed_cells(cases, groups, scores=None, index_info=None):
    """The cells a plan's census shows with a non-zero count.  `groups`: Plan.groups().  The batched count of a
    route = the jobs classified to it minus the jobs of its group(s).  align_band: a banded job that runs in the
    batch launch is settled there or finished behind it; which, the oracle's score says (scores[i] of case i)."""
    own = {}
    for g in groups:
        own[g["name"]] = own.get(g["name"], 0) + g["jobs"]
    routes = [(route_of(c, index_info) or (None,))[0] for c in cases]
    seen = set()
    for name in own:
        if name == BATCH:
            continue
        n = routes.count(name)
        if name == "align_band":
            if n - own[name] > 0:
                seen |= {name + ("/settled" if scores[i] <= ALIGN_BAND_HALF else "/unsettled")
                         for i, r in enumerate(routes) if r == name}
            continue
        if own[name] > 0:
            seen.add(name + "/own")
        if n - own[name] > 0:
            seen.add(name + "/batch")
    return seen
