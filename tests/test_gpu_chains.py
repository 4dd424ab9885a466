"""GPU: pgpu_index_refine_chains against what the reference's refinement loop left (the golden chains), against today's
two-call device route, and against the restatement (tests/chain_lib.py) -- never against the library under test alone.
Every comparison is byte equality."""
import ctypes as C

import numpy as np
import pytest

import chain_lib as CL
import refine_lib as RL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden(gpu_ctx):
    import pintron_amd.capi as capi
    gen, chains = CL.load_fixture()
    idx = capi.Index(gpu_ctx, gen)
    yield gen, chains, idx
    idx.close()


def triples(chains):
    return [(c["est"], c["exons"], c["settings"]) for c in chains]


def expect_arrays(exons, want):
    """want: per chain (status, done, dropped_first, exons afterwards, steps) -> the three arrays of the entry, over an
    output that starts as a copy of the input"""
    from pintron_amd import capi
    out_exons = exons.copy()
    out_steps = np.zeros(len(exons), dtype=np.uint8)
    res = np.zeros(len(want), dtype=np.dtype(capi.CHAIN_RESULT_DTYPE))
    k = 0
    for i, (status, done, dropped, ex2, steps) in enumerate(want):
        res[i] = (status, done, dropped, 0)
        for e, s in zip(ex2, steps):
            out_exons[k] = tuple(e)
            out_steps[k] = s
            k += 1
    assert k == len(exons)
    return out_exons, out_steps, res


def check(idx, ests, exons, q, want_arrays):
    out_exons, out_steps, res = idx.refine_chains(ests, exons, q)
    we, ws, wr = want_arrays
    for name, got, want in (("results", res, wr), ("steps", out_steps, ws), ("exons", out_exons, we)):
        if got.tobytes() != want.tobytes():
            bad = [i for i in range(len(got)) if got[i] != want[i]]
            raise AssertionError("%s differ at %d places, first %d: %r / %r" % (name, len(bad), bad[0], got[bad[0]], want[bad[0]]))
    return out_exons, out_steps, res


def test_every_golden_chain_in_one_call(golden):
    gen, chains, idx = golden
    ests, exons, q = CL.batch_arrays(triples(chains))
    want = [(CL.OK, c["done"], c["dropped_first"], c["exons_after"], c["steps"]) for c in chains]
    check(idx, ests, exons, q, expect_arrays(exons, want))
    assert idx.refine_chains_kernel_ms() > 0.0                 # the fixture's context has timing on


def test_golden_chains_by_the_two_call_route(golden, gpu_ctx):
    """per intron, a PGPU_DP_GAP plan on the chain's current windows followed by pgpu_index_refine_introns gives the same"""
    gen, chains, idx = golden
    ests, exons, q = CL.batch_arrays(triples(chains))
    out_exons, out_steps, res = idx.refine_chains(ests, exons, q)
    rounds = CL.device_rounds(gpu_ctx, idx, gen, triples(chains))
    k = 0
    for c, (ex2, steps) in zip(chains, rounds):
        n = len(c["exons"])
        assert [tuple(int(v) for v in e) for e in out_exons[k:k + n]] == ex2, c
        assert out_steps[k:k + n].tolist() == steps, c
        k += n


def test_hand_made_edges(golden, gpu_ctx, tmp_path):
    import pintron_amd.capi as capi
    L = capi.lib()
    gen, chains, idx = golden
    rng = np.random.default_rng(5)
    glen = len(gen)
    # a singleton; a chain at the very start and one at the very end of the sequence (windows clamped); exons nobody names
    e_lo = gen[0:40] + gen[300:340] + gen[700:750]
    lo = (e_lo, [(0, 39, 0, 39), (40, 79, 300, 339), (80, 129, 700, 749)], (30, 70, 30, 40))
    e_hi = gen[glen - 700:glen - 650] + gen[glen - 340:glen - 300] + gen[glen - 40:]
    hi = (e_hi, [(0, 49, glen - 700, glen - 651), (50, 89, glen - 340, glen - 301), (90, 129, glen - 40, glen - 1)], (30, 70, 30, 40))
    # borders a little off, so that the clamped windows are aligned and decided on
    lo2 = (e_lo, [(0, 36, 0, 36), (37, 82, 297, 342), (83, 129, 703, 749)], (30, 70, 30, 4))
    hi2 = (e_hi, [(0, 52, glen - 700, glen - 648), (53, 86, glen - 337, glen - 304), (87, 129, glen - 43, glen - 1)], (30, 70, 30, 4))
    # an intron so close to an end that a piece of its genomic window leaves the sequence: 70 bases in front of position
    # 50, 70 bases behind position glen - 40
    lo3 = (gen[0:20] + gen[50:90], [(0, 19, 0, 19), (20, 59, 50, 89)], (30, 70, 30, 4))
    hi3 = (gen[glen - 60:glen - 40] + gen[glen - 20:], [(0, 19, glen - 60, glen - 41), (20, 39, glen - 20, glen - 1)], (30, 70, 30, 4))
    for est, ex, st in (lo3, hi3):
        _, sg = RL.gap_windows(est, gen, ex[0], ex[1], *st[:3])
        assert len(sg) < 20 + 70 + 70 + 30                     # clamped indeed
    single = (chains[0]["est"], chains[0]["exons"][:1], chains[0]["settings"])
    some = triples(chains[:6])
    batch = [single, lo, hi, lo2, hi2, lo3, hi3] + some
    ests, exons, q = CL.batch_arrays(batch)
    # two exons no query names, one in front of every chain and one behind
    loose = np.array([(7, 9, 11, 13), (-1, -1, -1, -1)], dtype=exons.dtype)
    exons_l = np.concatenate([loose[:1], exons, loose[1:]])
    q_l = q.copy()
    q_l["first_exon"] += 1
    want = [CL.chain(est, gen, ex, st) for est, ex, st in batch]
    assert want[0][:3] == (CL.OK, 0, 0) and all(w[0] == CL.OK for w in want)
    we, ws, wr = expect_arrays(exons, want)
    check(idx, ests, exons, q, (we, ws, wr))
    check(idx, ests, exons_l, q_l, (np.concatenate([loose[:1], we, loose[1:]]), np.concatenate([[0], ws, [0]]).astype(np.uint8), wr))
    # an intron over each cap in the middle of a chain: `done` says where, the exons behind it are the input's, the chains
    # before and behind it are untouched.  The EST window: an unaligned stretch between the second and the third exon of
    # a golden chain whose exons are longer than the 30 bases a window takes of them -- 30 + 132 + 30 fits, 133 does not.
    c = next(c for c in chains if len(c["exons"]) >= 4 and not CL.has_est_gap(c["exons"]) and c["settings"][:3] == (30, 70, 30) and
             all(e[1] - e[0] >= 31 for e in c["exons"]) and all(s >> 7 for s in c["steps"][1:]))
    est, ex, st = c["est"], c["exons"], c["settings"]
    cut = ex[1][1] + 1
    for n_gap, status in ((CL.MAX_EST_WINDOW - 60, CL.OK), (CL.MAX_EST_WINDOW - 59, CL.ERANGE), (400, CL.ERANGE)):
        est2 = est[:cut] + RL.rnd(rng, n_gap) + est[cut:]
        ex2 = [e if k < 2 else (e[0] + n_gap, e[1] + n_gap, e[2], e[3]) for k, e in enumerate(ex)]
        batch = [some[0], (est2, ex2, st), some[1]]
        want = [CL.chain(e, gen, x, s) for e, x, s in batch]
        assert want[1][0] == status and want[0][0] == want[2][0] == CL.OK, (n_gap, want[1])
        if status == CL.ERANGE:
            assert want[1][1] == 1 and want[1][3][2:] == ex2[2:] and want[1][4][2:] == [0] * (len(ex) - 2)
        ests_b, exons_b, q_b = CL.batch_arrays(batch)
        check(idx, ests_b, exons_b, q_b, expect_arrays(exons_b, want))
    # the genomic window: 40 + 100 + 100 + 40, then 40 + 200 + 61, then 61 + 200 + 61 = 322
    wide_ex = [(0, 39, 5000, 5039), (40, 79, 5400, 5439), (80, 149, 5800, 5869), (150, 219, 6200, 6269)]
    wide = (b"".join(gen[e[2]:e[3] + 1] for e in wide_ex), wide_ex, (30, 100, 61, 4))
    batch = [some[2], wide, some[3]]
    want = [CL.chain(e, gen, x, s) for e, x, s in batch]
    assert want[1][:2] == (CL.ERANGE, 2) and want[1][3][3] == wide_ex[3], want[1]
    ests_b, exons_b, q_b = CL.batch_arrays(batch)
    check(idx, ests_b, exons_b, q_b, expect_arrays(exons_b, want))
    # every PGPU_EINVAL rule, against the restatement's verdict
    ests, exons, q = CL.batch_arrays(some)

    def rc_of(mod_q=None, mod_e=None, ests_=None):
        q2, e2 = q.copy(), exons.copy()
        if mod_q:
            mod_q(q2)
        if mod_e:
            mod_e(e2)
        b = ests if ests_ is None else ests_
        rc = idx.refine_chains_raw(b, e2, q2, len(q2))[0]
        assert (rc == capi.PGPU_EINVAL) == CL.einval(len(b), glen, e2, q2) and rc in (capi.PGPU_OK, capi.PGPU_EINVAL)
        return rc

    def put(field, i, value):
        def mod(x):
            x[field][i] = value
        return mod
    f1, n1 = int(q[1]["first_exon"]), int(q[1]["n_exons"])
    bad_q = [put("n_exons", 2, 0), put("n_exons", len(q) - 1, int(q[-1]["n_exons"]) + 1), put("first_exon", 3, len(exons)),
             put("first_exon", 3, 0xFFFFFFFF), put("est_off", 1, len(ests)), put("est_off", 1, 1 << 40), put("est_len", 1, 0xFFFFFFFF),
             put("est_len", 1, 0x80000000), put("reserved", 4, 1), put("first_exon", 1, f1 - 1), put("n_exons", 0, int(q[0]["n_exons"]) + 1),
             put("suffpref_length_on_est", 2, -1), put("suffpref_length_for_intron", 2, (1 << 24) + 1), put("suffpref_length_on_gen", 2, -7)]
    for k, mod in enumerate(bad_q):
        assert rc_of(mod_q=mod) == capi.PGPU_EINVAL, k
    bad_e = [put("EST_start", f1 + 1, -2), put("EST_end", f1 + 1, int(q[1]["est_len"]) + 1), put("GEN_start", f1 + 1, -2),
             put("GEN_end", f1 + 1, glen + 1), put("EST_end", f1, int(exons[f1 + 1]["EST_start"])),
             put("GEN_end", f1, int(exons[f1 + 1]["GEN_start"])), put("EST_start", f1 + n1 - 1, int(exons[f1 + n1 - 2]["EST_end"]))]
    for k, mod in enumerate(bad_e):
        assert rc_of(mod_e=mod) == capi.PGPU_EINVAL, k
    assert rc_of(ests_=ests[:-1]) == capi.PGPU_EINVAL                             # the last EST runs past the buffer
    assert rc_of(mod_q=put("min_intron_length", 2, -5)) == capi.PGPU_OK           # compared, never used as a length
    assert rc_of(mod_e=put("GEN_end", f1 + n1 - 1, glen)) == capi.PGPU_OK         # a coordinate may equal the length
    # null pointers and n == 0
    n_ex = len(exons)
    oe, os_, orr = np.zeros_like(exons), np.full(n_ex, 9, dtype=np.uint8), np.zeros(len(q), dtype=np.dtype(capi.CHAIN_RESULT_DTYPE))
    ep, qp = exons.ctypes.data_as(C.POINTER(capi.Factor)), q.ctypes.data_as(C.POINTER(capi.ChainQuery))
    oep, osp, orp = oe.ctypes.data_as(C.POINTER(capi.Factor)), os_.ctypes.data_as(C.POINTER(C.c_uint8)), orr.ctypes.data_as(C.POINTER(capi.ChainResult))
    f = L.pgpu_index_refine_chains
    assert f(gpu_ctx.h, None, ests, len(ests), ep, n_ex, qp, len(q), oep, osp, orp) == capi.PGPU_EINVAL
    assert f(gpu_ctx.h, idx.h, None, len(ests), ep, n_ex, qp, len(q), oep, osp, orp) == capi.PGPU_EINVAL
    assert f(gpu_ctx.h, idx.h, ests, len(ests), None, n_ex, qp, len(q), oep, osp, orp) == capi.PGPU_EINVAL
    assert f(gpu_ctx.h, idx.h, ests, len(ests), ep, n_ex, None, len(q), oep, osp, orp) == capi.PGPU_EINVAL
    assert f(gpu_ctx.h, idx.h, ests, len(ests), ep, n_ex, qp, len(q), None, osp, orp) == capi.PGPU_EINVAL
    assert f(gpu_ctx.h, idx.h, ests, len(ests), ep, n_ex, qp, len(q), oep, None, orp) == capi.PGPU_EINVAL
    assert f(gpu_ctx.h, idx.h, ests, len(ests), ep, n_ex, qp, len(q), oep, osp, None) == capi.PGPU_EINVAL
    assert f(gpu_ctx.h, idx.h, ests, len(ests), ep, n_ex, None, 0, oep, osp, None) == capi.PGPU_OK       # n == 0: a copy
    assert oe.tobytes() == exons.tobytes() and not os_.any()
    assert f(gpu_ctx.h, idx.h, None, 0, None, 0, None, 0, None, None, None) == capi.PGPU_OK
    want = [(CL.OK, c["done"], c["dropped_first"], c["exons_after"], c["steps"]) for c in chains[:6]]
    check(idx, ests, exons, q, expect_arrays(exons, want))                        # the context still answers
    # a loaded index
    path = str(tmp_path / "chains.idx")
    idx.save(path)
    loaded = capi.Index(gpu_ctx, gen, load_from=path)
    check(loaded, ests, exons, q, expect_arrays(exons, want))
    loaded.close()


def test_kernel_ms_is_zero_without_timing(golden):
    import pintron_amd.capi as capi
    gen, chains, _ = golden
    ests, exons, q = CL.batch_arrays(triples(chains[:50]))
    with capi.Context(0) as ctx:
        idx = capi.Index(ctx, gen)
        idx.refine_chains(ests, exons, q)
        assert idx.refine_chains_kernel_ms() > 0.0
        ctx.L.pgpu_set_timing(ctx.h, 0)
        idx.refine_chains(ests, exons, q)
        assert idx.refine_chains_kernel_ms() == 0.0
        idx.close()


BATCH, DISTINCT, SAMPLE = 100_000, 12_500, 10_000


def test_a_hundred_thousand_generated_chains_in_one_call(golden):
    """one batch of 100 000 chains: 12 500 generated factorizations of two to six exons, planted at random places of a
    copy of the sequence, each under eight settings (two window triples, four min_intron_length).  The restatement is
    a Python loop: a seeded sample of 10 000 chains is compared, and every result must be a well-formed one."""
    import pintron_amd.capi as capi
    gen, _, _ = golden
    rng = np.random.default_rng(2024)
    g = bytearray(gen[:400_000])
    bases = []
    pos = 300
    while len(bases) < DISTINCT:
        made = CL.make_chain(rng, g, pos, int(rng.integers(2, 7)))
        if made is None:
            pos = 300 + int(rng.integers(0, 5000)) if pos + 9000 > len(g) else pos + 1
            continue
        est, exons, st, _, end = made
        bases.append((est, exons, st))
        pos = end + 21 if end + 9000 < len(g) else 300 + int(rng.integers(0, 5000))      # later rounds plant over earlier ones
    g = bytes(g)
    batch = []
    for est, exons, st in bases:
        ilen = exons[1][2] - exons[0][3] - 1
        for sp in (st[:3], (30, 70, 30) if st[:3] != (30, 70, 30) else (25, 60, 35)):
            for mil in (4, 40, ilen, ilen + 25):
                batch.append((est, exons, sp + (mil,)))
    assert len(batch) == BATCH
    ests, exons, q = CL.batch_arrays(batch)
    with capi.Context(0) as ctx:
        idx = capi.Index(ctx, g)
        out_exons, out_steps, res = idx.refine_chains(ests, exons, q)
        idx.close()
    assert np.all(res["pad"] == 0) and np.all((res["status"] == CL.OK) | (res["status"] == CL.ERANGE))
    assert np.all(res["done"][res["status"] == CL.OK] == q["n_exons"][res["status"] == CL.OK] - 1)
    assert np.all((out_steps & 0x70) == 0) and np.all((out_steps & 15) < RL.N_PATHS)
    sample = np.sort(rng.permutation(BATCH)[:SAMPLE])
    seen_first, seen_later, dropped = set(), set(), 0
    for i in sample:
        est, ex, st = batch[int(i)]
        status, done, drop, ex2, steps = CL.chain(est, g, ex, st)
        k, n = int(q[i]["first_exon"]), len(ex)
        got = (int(res[i]["status"]), int(res[i]["done"]), int(res[i]["dropped_first"]),
               [tuple(int(v) for v in e) for e in out_exons[k:k + n]], out_steps[k:k + n].tolist())
        assert got == (status, done, drop, ex2, steps), (int(i), got, (status, done, drop, ex2, steps))
        seen_first |= {s & 15 for s in steps[1:2]}
        seen_later |= {s & 15 for s in steps[2:]}
        dropped += drop
    assert len(seen_first) >= 8 and len(seen_later) >= 8 and dropped > 0, (seen_first, seen_later, dropped)
