"""GPU: pgpu_index_refine_introns against what the reference's refine_intron returned (the golden cases) and against
the restatement of the decision (tests/refine_lib.py) -- never against the library under test.  Every field of every
result must match."""
import ctypes as C

import numpy as np
import pytest

import refine_lib as RL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden(gpu_ctx):
    import pintron_amd.capi as capi
    gen, cases = RL.load_fixture()
    idx = capi.Index(gpu_ctx, gen)
    yield gen, cases, idx
    idx.close()


def expect_of(c):
    return (RL.OK, c["refined"], c["path"], c["donor_after"], c["acceptor_after"])


def check(idx, ests, rows, q, want):
    res = idx.refine_introns(ests, rows, q)
    assert len(res) == len(want)
    for i, w in enumerate(want):
        assert int(res[i]["pad"]) == 0
        assert RL.result_tuple(res[i]) == w, (i, RL.result_tuple(res[i]), w, q[i])
    return res


def test_golden_cases_with_the_oracles_rows(golden, O):
    """(a) every golden case, rows from the oracle's CPU gap alignment"""
    gen, cases, idx = golden
    items = []
    for c in cases:
        er, gr, v = RL.oracle_rows(O, c["est"], gen, c["donor"], c["acceptor"], *c["settings"][:3])
        items.append((c["est"], er, gr, v, c["donor"], c["acceptor"], c["first"], c["settings"]))
    ests, rows, q = RL.query_array(items)
    check(idx, ests, rows, q, [expect_of(c) for c in cases])
    assert idx.refine_introns_kernel_ms() > 0.0               # the fixture's context has timing on


def test_golden_cases_behind_a_device_gap_plan(golden, gpu_ctx):
    """(b) the composition a caller uses: rows and v[1..5] from a PGPU_DP_GAP plan, then the new call"""
    import pintron_amd.capi as capi
    gen, cases, idx = golden
    jl = capi.JobList()
    for c in cases:
        se, sg = RL.gap_windows(c["est"], gen, c["donor"], c["acceptor"], *c["settings"][:3])
        jl.add(capi.GAP, se, sg)
    out = capi.run_jobs(gpu_ctx, jl)
    items = []
    for c, o in zip(cases, out):
        assert o["status"] == 0
        v = (o["factor_cut"], o["intron_start"], o["intron_end"], o["intron_start_on_align"], o["intron_end_on_align"])
        assert len(o["ea"]) == len(o["ga"]) == o["dim"]
        items.append((c["est"], o["ea"], o["ga"], v, c["donor"], c["acceptor"], c["first"], c["settings"]))
    ests, rows, q = RL.query_array(items)
    check(idx, ests, rows, q, [expect_of(c) for c in cases])


def restate(gen, items):
    return [RL.refine(est, gen, er, gr, v, d, a, first, *st) for est, er, gr, v, d, a, first, st in items]


def hand_item(gen, est_row, gen_row, isoa, ieoa, est=None, shift=0, first=False, mil=4, base=5000, intron=900):
    """a query over hand-made rows: the donor ends where the rows' intron starts, on a fixed stretch of the sequence;
    the EST defaults to the ungapped EST row between 64 bases of padding"""
    pre_e = sum(1 for x in est_row[:isoa] if x not in (45, 0))
    pre_g = sum(1 for x in gen_row[:isoa] if x not in (45, 0))
    mid = sum(1 for x in gen_row[isoa:ieoa + 1] if x not in (45, 0))
    if est is None:
        est = b"A" * 64 + bytes(x for x in est_row if x not in (45, 0)) + b"T" * 64
    donor = (64, 64 + pre_e - 1 + shift, base, base + pre_g - 1)
    acceptor = (64 + pre_e + shift, len(est) - 40, base + pre_g + intron, base + pre_g + intron + 60)
    v = (pre_e, pre_g, pre_g + mid - 1 if mid else pre_g, isoa, ieoa)
    # the rows stand for windows of 30 + gap + 30 against 30 + mid / 2 + mid / 2 + 30
    return (est, bytes(est_row), bytes(gen_row), v, donor, acceptor, first, (30, mid // 2, 30, mil))


def test_hand_made_rows(golden):
    """(c) rows the alignment would not make, against the restatement"""
    import pintron_amd.capi as capi
    gen, _, idx = golden
    rng = np.random.default_rng(77)
    g0 = gen[5000 - 30:5000]
    items, names = [], []

    def add(name, *a, **k):
        names.append(name)
        items.append(hand_item(gen, *a, **k))
    mid = b"CCTTTTCCTTCCTTTTCCTTCCTCCCTTCC"                 # 30 intron columns without a site
    add("rows begin and end in '-'", b"CC" + g0 + b"-" * 30 + b"TTCAGTTCAG--", b"--" + g0 + mid + b"TTCAGTTCAGCC", 32, 61)
    add("AG only in the last two columns", g0 + b"-" * 30 + b"TTCCTTCCAG", g0 + mid + b"TTCCTTCCAG", 30, 59)
    add("init at column 0", b"-" * 30 + b"TTCAGTTCAG", mid + b"TTCAGTTCAG", 0, 29)
    add("init at column 0, first intron", b"-" * 30 + b"TTCAGTTCAG", mid + b"TTCAGTTCAG", 0, 29, first=True)
    add("intron starts at column 1", b"G" + b"-" * 30 + b"TTCAGTTCAG", b"G" + mid + b"TTCAGTTCAG", 1, 30)
    for er, gr in ((b"A", b"A"), (b"-", b"G"), (b"AG", b"AG"), (b"G-", b"GT"), (b"-G", b"AG")):
        add("dim %d" % len(gr), er, gr, 0, len(gr) - 1)
        add("dim %d, later column" % len(gr), er, gr, len(gr) - 1, len(gr) - 1, shift=1)
    add("sites split by gap columns", g0[:26] + b"CCGGC-T--" + b"-" * 30 + b"TTCA--GTTCAG", g0[:26] + b"CC-G--TCC" + mid + b"TTCA--GTTCAG", 35, 64)
    add("GC split by gap columns", g0[:26] + b"CCGGC-T--" + b"-" * 30 + b"TTCA--GTTCAG", g0[:26] + b"CC-G--CCC" + mid + b"TTCA--GTTCAG", 35, 64)
    add("a NUL inside the rows", g0 + b"-" * 30 + b"TTC\0GTTCAG", g0 + mid + b"TTCA\0TTCAG", 30, 59)
    add("an empty genomic row", b"ACGT", b"\0CGT", 1, 2)
    # dim at and above PGPU_REFINE_MAX_DIM
    for dim in (RL.MAX_DIM - 1, RL.MAX_DIM, RL.MAX_DIM + 1, RL.MAX_DIM + 500):
        tail = RL.rnd(rng, dim - 60)
        add("dim %d" % dim, g0 + b"-" * 30 + tail, g0 + mid + tail, 30, 59)
    # an operand of an edit distance at and above the cap: the first AG lies L columns behind the intron, so the EST
    # piece that is cut has L bytes (less the EST row's gaps) and the genomic one L (less the genomic row's)
    for L, egaps, ggaps in ((256, 0, 0), (257, 0, 0), (257, 1, 0), (257, 0, 1), (257, 1, 1), (258, 1, 1), (255, 0, 0), (258, 2, 0), (258, 0, 2)):
        body = bytearray(b"CT" * 200)[:L - 2] + b"AG"
        er, gr = bytearray(body), bytearray(body)
        for k in range(egaps):
            er[10 + k] = 45
        for k in range(ggaps):
            gr[20 + k] = 45
        est = b"A" * 64 + g0 + bytes(x for x in er if x != 45) + b"CTCTCTCTCT" + b"T" * 64
        add("operands %d / %d" % (L - egaps, L - ggaps), g0 + b"-" * 30 + bytes(er) + b"CTCTCTCTCT", g0 + mid + bytes(gr) + b"CTCTCTCTCT", 30, 59, est=est)
    # unsigned wrap in the _1 rule: the EST continues as the intron does (distance 0 to the shifted piece) and not as
    # the acceptor (distance 1..5 to the piece it leaves): 0 - edit_prev wraps
    for k in (2, 3, 4, 5):
        ins = gen[5030:5030 + k]                                # the intron's first bytes on the sequence
        acc = bytes(b"ACGT"[(b"ACGT".index(x) + 1) % 4] for x in ins[:k - 2]) + b"AG"
        est = b"A" * 64 + g0 + ins + b"CTCTCTCTCTCTCTCTCTCT" + b"T" * 64
        add("wrap, %d bases" % k, g0 + b"-" * 30 + ins + b"CTCTCTCTCT", g0 + ins + b"GT" + mid[k + 2:] + acc + b"CTCTCTCTCT", 30, 59, est=est)
    before = RL.STATS["wrapped"]
    want = restate(gen, items)
    assert RL.STATS["wrapped"] > before                       # the wrap did happen in the restatement
    by_name = dict(zip(names, want))
    assert by_name["dim %d" % RL.MAX_DIM][0] == RL.OK and by_name["dim %d" % (RL.MAX_DIM + 1)][0] == RL.ERANGE
    assert by_name["operands 256 / 256"][0] == RL.OK and by_name["operands 255 / 255"][0] == RL.OK
    for nm in ("operands 257 / 257", "operands 256 / 257", "operands 257 / 256", "operands 258 / 256", "operands 256 / 258"):
        assert by_name[nm][0] == RL.ERANGE, (nm, by_name[nm])
    assert by_name["operands 256 / 256"][2] >= 5 and by_name["operands 257 / 257"][1:3] == (0, 0)
    ests, rows, q = RL.query_array(items)
    res = idx.refine_introns(ests, rows, q)
    for i, w in enumerate(want):
        assert RL.result_tuple(res[i]) == w, (names[i], RL.result_tuple(res[i]), w)
    # random rows over a small alphabet rich in sites, every intron position
    items = []
    for _ in range(4000):
        dim = int(rng.integers(1, 90))
        letters = np.frombuffer(b"AGGTC-AG-T", dtype=np.uint8)
        gr = letters[rng.integers(0, len(letters), dim)].tobytes()
        er = bytes(x if rng.random() < 0.8 else int(letters[rng.integers(len(letters))]) for x in gr)
        isoa = int(rng.integers(0, dim))
        ieoa = int(rng.integers(isoa, dim))
        items.append(hand_item(gen, er, gr, isoa, ieoa, shift=int(rng.integers(0, 3)), first=bool(rng.integers(2)),
                               base=int(rng.integers(3000, 9000)), intron=int(rng.integers(100, 400))))
    want = restate(gen, items)
    assert len({w[2] for w in want}) >= 8                     # they reach most branches
    ests, rows, q = RL.query_array(items)
    check(idx, ests, rows, q, want)


def test_error_table_and_a_loaded_index(golden, gpu_ctx, O, tmp_path):
    """(d) every PGPU_EINVAL cause, n == 0, a loaded index"""
    import pintron_amd.capi as capi
    L = capi.lib()
    gen, cases, idx = golden
    items = []
    for c in cases[:40]:
        er, gr, v = RL.oracle_rows(O, c["est"], gen, c["donor"], c["acceptor"], *c["settings"][:3])
        items.append((c["est"], er, gr, v, c["donor"], c["acceptor"], c["first"], c["settings"]))
    want = [expect_of(c) for c in cases[:40]]
    ests, rows, q = RL.query_array(items)
    check(idx, ests, rows, q, want)

    def rc_of(mod, ests_=None, rows_=None):
        q2 = q.copy()
        mod(q2)
        return idx.refine_introns_raw(ests if ests_ is None else ests_, rows if rows_ is None else rows_, q2, len(q2))[0]

    def put(field, i, value, sub=None):
        def mod(x):
            if sub is None:
                x[field][i] = value
            else:
                x[field][sub][i] = value
        return mod
    last = len(q) - 1
    bad = [put("est_off", 3, len(ests) - 2), put("est_off", 3, 1 << 40), put("est_len", 3, 0xFFFFFFFF),
           put("rows_off", last, len(rows) - 2 * int(q[last]["dim"]) + 1), put("rows_off", 5, 1 << 41), put("dim", last, 0x7FFFFFFF),
           put("flags", 7, 2), put("flags", 7, 0x80000001), put("dim", 9, 0),
           put("donor", 11, int(q[11]["acceptor"]["EST_start"]), "EST_end"), put("donor", 11, int(q[11]["acceptor"]["GEN_start"]), "GEN_end"),
           put("acceptor", 11, int(q[11]["donor"]["EST_end"]), "EST_start"),
           put("donor", 13, -2, "EST_start"), put("acceptor", 13, len(gen) + 1, "GEN_end"), put("acceptor", 13, int(q[13]["est_len"]) + 1, "EST_end"),
           put("factor_cut", 15, -1), put("intron_end_on_align", 15, int(q[15]["dim"]) + 1), put("suffpref_length_for_intron", 17, -1)]
    for k, mod in enumerate(bad):
        assert rc_of(mod) == capi.PGPU_EINVAL, k
    assert rc_of(lambda x: None, ests_=ests[:-1]) == capi.PGPU_EINVAL            # the last EST runs past the buffer
    assert rc_of(lambda x: None, rows_=rows[:-1]) == capi.PGPU_EINVAL
    assert rc_of(put("min_intron_length", 2, -5)) == capi.PGPU_OK                 # compared, never used as a length
    r = (capi.RefineResult * len(q))()
    qp = q.ctypes.data_as(C.POINTER(capi.RefineQuery))
    args = (ests, len(ests), rows, len(rows))
    assert L.pgpu_index_refine_introns(gpu_ctx.h, idx.h, *args, None, len(q), r) == capi.PGPU_EINVAL
    assert L.pgpu_index_refine_introns(gpu_ctx.h, idx.h, *args, qp, len(q), None) == capi.PGPU_EINVAL
    assert L.pgpu_index_refine_introns(gpu_ctx.h, None, *args, qp, len(q), r) == capi.PGPU_EINVAL
    assert L.pgpu_index_refine_introns(gpu_ctx.h, idx.h, None, len(ests), rows, len(rows), qp, len(q), r) == capi.PGPU_EINVAL
    assert L.pgpu_index_refine_introns(gpu_ctx.h, idx.h, ests, len(ests), None, len(rows), qp, len(q), r) == capi.PGPU_EINVAL
    assert L.pgpu_index_refine_introns(gpu_ctx.h, idx.h, *args, None, 0, None) == capi.PGPU_OK      # n == 0
    assert L.pgpu_index_refine_introns(gpu_ctx.h, idx.h, None, 0, None, 0, None, 0, None) == capi.PGPU_OK
    check(idx, ests, rows, q, want)                                               # the context still answers
    path = str(tmp_path / "refine.idx")
    idx.save(path)
    loaded = capi.Index(gpu_ctx, gen, load_from=path)
    check(loaded, ests, rows, q, want)
    loaded.close()


BATCH, DISTINCT, SAMPLE = 100_000, 12_500, 25_000


def test_a_hundred_thousand_random_queries_in_one_call(golden, O):
    """(e) one batch of 100 000 queries: 12 500 generated introns (at the fixture's planted sites and at random places
    of the sequence, where no site was planted), each under eight settings (first / later intron, four
    min_intron_length).  The restatement is a Python loop: a random SAMPLE of 25 000 queries is compared (about 20 s), and every
    result must be a well-formed one."""
    gen, cases, idx = golden
    rng = np.random.default_rng(99)
    bases = []
    while len(bases) < DISTINCT:
        if rng.random() < 0.5:
            c0 = cases[int(rng.integers(len(cases)))]
            c = dict(ds=c0["donor"][2], de=c0["donor"][3], as_=c0["acceptor"][2], ae=c0["acceptor"][3])
            if not (c["ds"] + 5 < c["de"] < c["as_"] - 30 and c["as_"] + 5 < c["ae"]):
                continue
        else:
            c = RL.make_case(rng, int(rng.integers(200, len(gen) - 2000)))
        case = RL.finish_case(rng, gen, c)
        if case is None:
            continue
        est, donor, acceptor, _, st = case
        er, gr, v = RL.oracle_rows(O, est, gen, donor, acceptor, *st[:3])
        bases.append((est, er, gr, v, donor, acceptor, st))
    items = []
    for est, er, gr, v, donor, acceptor, st in bases:
        ilen = acceptor[2] - donor[3] - 1
        for first in (False, True):
            for mil in (4, 40, ilen, ilen + 25):
                items.append((est, er, gr, v, donor, acceptor, first, st[:3] + (mil,)))
    assert len(items) == BATCH
    ests, rows, q = RL.query_array(items)
    res = idx.refine_introns(ests, rows, q)
    assert len(res) == BATCH
    assert np.all(res["pad"] == 0) and np.all((res["status"] == RL.OK) | (res["status"] == RL.ERANGE))
    assert np.all((res["path"] >= 0) & (res["path"] < RL.N_PATHS)) and np.all((res["refined"] == 0) | (res["refined"] == 1))
    sample = rng.permutation(BATCH)[:SAMPLE]
    seen = set()
    for i in sample:
        est, er, gr, v, donor, acceptor, first, st = items[int(i)]
        w = RL.refine(est, gen, er, gr, v, donor, acceptor, first, *st)
        assert RL.result_tuple(res[int(i)]) == w, (int(i), RL.result_tuple(res[int(i)]), w)
        seen.add(w[2])
    assert len(seen) >= 8, seen
