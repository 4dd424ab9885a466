"""CPU restatement of pgpu_index_refine_chains: the reference's refinement loop over one factorization
(src/est-factorizations.c:446-490) with the windows, the gap alignment and the border decision of every intron.

chain           the loop in Python: refine_lib.gap_windows -> oracle_lib.gap_align -> refine_lib.refine per intron, on the
                exons as they are at that moment, then the first-exon rule (:476-485); the caps of the entry.
solo            every intron refined alone from the ORIGINAL exons: what a caller gets who does not chain.
einval          the PGPU_EINVAL rules of the entry for one call.
RefChain        the same loop over refine_intron of the reference's object code (oracle/_ref, through
                refine_lib.RefRefiner), one forked child per chain.
make_chain      generated factorizations: the planted introns of refine_lib.make_case strung into multi-exon ESTs, the
                noise of refine_lib.finish_case at every junction.
load_fixture    tests/golden/refine_chains.json.gz (tools/make_chain_golden.py).
"""
import gzip
import json
import os

import numpy as np

import oracle_lib as O
import refine_lib as RL

FIXTURE = os.path.join(RL.ROOT, "tests", "golden", "refine_chains.json.gz")
MAX_EST_WINDOW = 192      # PGPU_CHAIN_MAX_EST_WINDOW
MAX_GEN_WINDOW = 320      # PGPU_CHAIN_MAX_GEN_WINDOW
OK, ERANGE, EINVAL = 0, -34, -22
# the branches an intron of a chain can take: `attached-first` (path 0, :127-135) needs first_intron, which the loop sets
# for the chain's first intron alone, and `attached-later` (path 1, :136-140) needs it unset
PATHS_FIRST = (0, 2, 3, 4, 5, 6, 7, 8, 9)
PATHS_LATER = (1, 2, 3, 4, 5, 6, 7, 8, 9)


def step_byte(refined, path):
    return path | (refined << 7)


def chain(est: bytes, gen: bytes, exons, settings, info=None):
    """One query -> (status, done, dropped_first, exons afterwards, steps).  exons: [(EST_start, EST_end, GEN_start,
    GEN_end)]; settings = (suffpref_length_on_est, _for_intron, _on_gen, min_intron_length).  `info` (a dict) receives
    "outside" (a scan of some intron left its rows: the reference is not defined there) and "windows", the (EST window,
    genomic window, donor, acceptor) of every intron that was aligned."""
    sp_est, sp_int, sp_gen, mil = settings
    ex = [tuple(int(v) for v in e) for e in exons]
    steps = [0] * len(ex)
    outside, windows = False, []
    status, done = OK, 0
    for i in range(len(ex) - 1):
        donor, acceptor = ex[i], ex[i + 1]
        se, sg = RL.gap_windows(est, gen, donor, acceptor, sp_est, sp_int, sp_gen)
        if len(se) > MAX_EST_WINDOW or len(sg) > MAX_GEN_WINDOW:
            status = ERANGE
            break
        r = O.gap_align(se, sg)
        v = (r["factor_cut"], r["intron_start"], r["intron_end"], r["intron_start_on_align"], r["intron_end_on_align"])
        one = {}
        st, refined, path, d2, a2 = RL.refine(est, gen, r["ea"], r["ga"], v, donor, acceptor, i == 0, sp_est, sp_int, sp_gen, mil,
                                              info=one)
        if st != RL.OK:                                # an operand of an edit distance beyond PGPU_REFINE_MAX_ED
            status = ERANGE
            break
        outside |= one.get("outside", False)
        windows.append((se, sg, donor, acceptor))
        ex[i], ex[i + 1] = d2, a2
        steps[i + 1] = step_byte(refined, path)
        done = i + 1
    dropped = int(status == OK and len(ex) > 1 and ex[0][0] == ex[1][0])
    if info is not None:
        info["outside"], info["windows"] = outside, windows
    return status, done, dropped, ex, steps


def solo(est: bytes, gen: bytes, exons, settings):
    """every intron refined alone from the original exons, the answers put together exon by exon -> (exons, steps); None
    for an intron beyond the caps"""
    ex = [tuple(int(v) for v in e) for e in exons]
    out = [list(e) for e in ex]
    steps = [0] * len(ex)
    for i in range(len(ex) - 1):
        one = _one(est, gen, ex[i], ex[i + 1], i == 0, settings)
        if one is None:
            return None
        refined, path, d2, a2 = one
        out[i][1], out[i][3] = d2[1], d2[3]
        out[i + 1][0], out[i + 1][2] = a2[0], a2[2]
        steps[i + 1] = step_byte(refined, path)
    return [tuple(e) for e in out], steps


def _one(est, gen, donor, acceptor, first, settings):
    """one intron on its own -> (refined, path, donor, acceptor), None beyond the caps"""
    sp_est, sp_int, sp_gen, mil = settings
    se, sg = RL.gap_windows(est, gen, donor, acceptor, sp_est, sp_int, sp_gen)
    if len(se) > MAX_EST_WINDOW or len(sg) > MAX_GEN_WINDOW:
        return None
    r = O.gap_align(se, sg)
    v = (r["factor_cut"], r["intron_start"], r["intron_end"], r["intron_start_on_align"], r["intron_end_on_align"])
    st, refined, path, d2, a2 = RL.refine(est, gen, r["ea"], r["ga"], v, donor, acceptor, first, sp_est, sp_int, sp_gen, mil)
    return None if st != RL.OK else (refined, path, d2, a2)


def is_a_chain(est, gen, exons, settings, answer):
    """the chain's answer (exons afterwards, steps) differs from refining every intron alone from the original exons"""
    alone = solo(est, gen, exons, settings)
    return alone is not None and (list(alone[0]), list(alone[1])) != (list(answer[0]), list(answer[1]))


def has_est_gap(exons):
    return any(b[0] - a[1] - 1 > 0 for a, b in zip(exons, exons[1:]))


def odd_bases_near_a_junction(est, exons, reach=15):
    """a byte that is no upper-case A, C, G or T within `reach` bases of a junction of the original factorization"""
    for a in exons[:-1]:
        lo = max(0, a[1] - reach)
        if any(x not in b"ACGT" for x in est[lo:a[1] + reach + 1]):
            return True
    return False


# ---- the PGPU_EINVAL rules ------------------------------------------------------------------------------------------
def einval(ests_len, gen_len, exons, queries):
    """True when pgpu_index_refine_chains refuses the whole call.  exons: array or list of 4-tuples; queries: records or
    dicts with the fields of pgpu_chain_query."""
    named = set()
    for q in queries:
        est_off, est_len, first, n = int(q["est_off"]), int(q["est_len"]), int(q["first_exon"]), int(q["n_exons"])
        if est_off > ests_len or est_len > ests_len - est_off or est_len > 0x7FFFFFFF or int(q["reserved"]) != 0:
            return True
        if n == 0 or first > len(exons) or n > len(exons) - first:
            return True
        for f in ("suffpref_length_on_est", "suffpref_length_for_intron", "suffpref_length_on_gen"):
            if not 0 <= int(q[f]) <= 1 << 24:
                return True
        for k in range(first, first + n):
            if k in named:
                return True
            named.add(k)
            es, ee, gs, ge = (int(v) for v in exons[k])
            if not (-1 <= es <= est_len and -1 <= ee <= est_len and -1 <= gs <= gen_len and -1 <= ge <= gen_len):
                return True
            if k + 1 < first + n:                      # the my_asserts of :52-53
                nes, _, ngs, _ = (int(v) for v in exons[k + 1])
                if ee >= nes or ge >= ngs:
                    return True
    return False


# ---- the reference's object code ------------------------------------------------------------------------------------
class RefChain:
    """the loop of src/est-factorizations.c:446-490 over refine_intron of the reference's object code; one forked child per
    chain, for the reference's Shift_* routines overrun heap blocks on some inputs"""

    def __init__(self, gen: bytes):
        self.ref = RL.RefRefiner(gen)

    @property
    def gen(self):
        return self.ref.gen

    def _loop(self, est, exons, settings):
        ex = [tuple(e) for e in exons]
        returned = [0] * len(ex)
        for i in range(len(ex) - 1):
            refined, d2, a2 = self.ref.refine(est, ex[i], ex[i + 1], i == 0, *settings)
            ex[i], ex[i + 1] = tuple(d2), tuple(a2)
            returned[i + 1] = refined
        dropped = int(len(ex) > 1 and ex[0][0] == ex[1][0])
        return dropped, ex, returned

    def run(self, est: bytes, exons, settings):
        """-> (dropped_first, exons afterwards, refine_intron's return values per exon) or None when the child dies"""
        r, w = os.pipe()
        pid = os.fork()
        if pid == 0:
            try:
                os.close(r)
                os.write(w, json.dumps(self._loop(est, exons, settings)).encode())
            finally:
                os._exit(0)
        os.close(w)
        data = b""
        while True:
            chunk = os.read(r, 65536)
            if not chunk:
                break
            data += chunk
        os.close(r)
        _, st = os.waitpid(pid, 0)
        if st != 0 or not data:
            return None
        dropped, ex, returned = json.loads(data)
        return dropped, [tuple(e) for e in ex], returned


# ---- generated inputs -----------------------------------------------------------------------------------------------
AIMS = (None, None, None, "attached", "refused-acceptor", "refused-donor", "repeat-left", "repeat-right", "gc-left")


def plan_chain(rng, pos, n_exons, aims=None):
    """n_exons - 1 planted introns (refine_lib.make_case), the acceptor exon of one the donor exon of the next:
    (exon extents on the sequence [(start, end)], edits [(pos, bytes)], aims)"""
    extents, edits, used = [], [], []
    p = pos
    for j in range(n_exons - 1):
        aim = aims[j] if aims is not None else AIMS[int(rng.integers(len(AIMS)))]
        kind = int(rng.integers(10))
        if aim == "gc-left" or kind < 2:
            c = RL.make_case(rng, p, site=(b"GC", b"AG"), short_exons=kind == 0, aim=aim)
        elif kind == 2:
            c = RL.make_case(rng, p, site=None, aim=aim)
        else:
            c = RL.make_case(rng, p, short_exons=kind == 3, aim=aim)
        extents.append((p, c["de"]))
        edits += c["edits"]
        used.append(aim)
        p = c["as_"]
        last = c["ae"]
    extents.append((p, last))
    return extents, edits, used


def finish_chain(rng, gen, extents, aims):
    """the EST and the factors of a planted chain over the edited sequence: the exons joined between 64 bases of padding,
    at every junction the noise of refine_lib.finish_case (a substitution, an indel, an N, lower case, an unaligned gap)
    and a border the factorization has moved -> (est, exons, settings) or None"""
    parts = [bytearray(gen[s:e + 1]) for s, e in extents]
    for j, aim in enumerate(aims):
        if aim == "attached":                           # the donor's bases continue the acceptor exon to the left
            s2 = extents[j + 1][0]
            parts[j] = bytearray(gen[s2 - len(parts[j]):s2])
    gaps, moves = [], []
    for j in range(len(parts) - 1):
        ex1, ex2 = parts[j], parts[j + 1]
        r = rng.random()
        near1 = max(0, len(ex1) - 1 - int(rng.integers(0, 12)))
        near2 = min(len(ex2) - 1, int(rng.integers(0, 12)))
        if r < 0.15:
            ex1[near1] = b"ACGT"[int(rng.integers(4))]
        elif r < 0.28:
            ex2[near2] = b"ACGT"[int(rng.integers(4))]
        elif r < 0.34 and len(ex1) > 4:
            del ex1[near1]
        elif r < 0.40:
            ex2.insert(near2, b"ACGT"[int(rng.integers(4))])
        elif r < 0.46:
            ex1[near1] = ord("N")
        elif r < 0.52:
            ex2[near2:near2 + 3] = bytes(ex2[near2:near2 + 3]).lower()
        gaps.append(RL.rnd(rng, int(rng.integers(1, 7))) if rng.random() < 0.06 else b"")
        u = rng.random()
        if aims[j] is not None or u < 0.25:
            m = 0 if aims[j] is not None and u < 0.7 else int(rng.integers(0, 4))
        elif u < 0.8:
            m = int(rng.integers(1, 10))
        else:
            m = int(rng.integers(0, 26))
        moves.append(-m if rng.random() < 0.5 else m)
    est = bytearray(b"A" * 64)
    at = []
    for j, p in enumerate(parts):
        at.append((len(est), len(est) + len(p) - 1))
        est += p
        if j < len(gaps):
            est += gaps[j]
    est += b"T" * 64
    ex = [[at[j][0], at[j][1], extents[j][0], extents[j][1]] for j in range(len(parts))]
    for j, m in enumerate(moves):
        if gaps[j]:
            ex[j][1] += min(m, 0)
            ex[j + 1][0] += max(m, 0)
        else:
            ex[j][1] += m
            ex[j + 1][0] += m
        ex[j][3] += m
        ex[j + 1][2] += m
        if rng.random() < 0.2:                          # the two borders disagree by a little
            ex[j][3] += int(rng.integers(-3, 4))
        if rng.random() < 0.12:
            ex[j + 1][2] += int(rng.integers(-3, 4))
    for j, e in enumerate(ex):
        if not (e[0] <= e[1] and e[2] <= e[3]):
            return None
        if j and not (ex[j - 1][1] < e[0] and ex[j - 1][3] < e[2]):
            return None
    if rng.random() < 0.8:
        sp = (30, 70, 30)
    else:
        sp = (int(rng.integers(8, 41)), int(rng.integers(10, 91)), int(rng.integers(8, 41)))
    j = int(rng.integers(len(ex) - 1))
    ilen = ex[j + 1][2] - ex[j][3] - 1
    mil = (40, 40, 40, 4, 60, ilen, ilen + 2)[int(rng.integers(7))]
    return bytes(est), [tuple(e) for e in ex], sp + (mil,)


def make_chain(rng, gen: bytearray, pos, n_exons, aims=None):
    """plants a chain at `pos` of the (mutable) sequence -> (est, exons, settings, edits, end) or None (the sequence
    then is as before)"""
    extents, edits, used = plan_chain(rng, pos, n_exons, aims)
    if extents[-1][1] + 200 > len(gen):
        return None
    saved = [(p, bytes(gen[p:p + len(s)])) for p, s in edits]
    for p, s in edits:
        gen[p:p + len(s)] = s
    case = finish_chain(rng, gen, extents, used)
    if case is None:
        for p, s in reversed(saved):
            gen[p:p + len(s)] = s
        return None
    return case + (edits, extents[-1][1])


def batch_arrays(chains):
    """chains of (est, exons, settings) -> (ests, exons array, queries array) in the layouts of the entry; equal ESTs are
    stored once"""
    from pintron_amd import capi
    n_ex = sum(len(c[1]) for c in chains)
    exons = np.zeros(n_ex, dtype=np.dtype(capi.FACTOR_DTYPE))
    q = np.zeros(len(chains), dtype=np.dtype(capi.CHAIN_QUERY_DTYPE))
    ests, eat, eoff, k = [], {}, 0, 0
    for i, (est, ex, st) in enumerate(chains):
        if est not in eat:
            eat[est] = eoff
            ests.append(est)
            eoff += len(est)
        for e in ex:
            exons[k] = tuple(e)
            k += 1
        q[i] = (eat[est], len(est), k - len(ex), len(ex), 0) + tuple(st)
    return b"".join(ests), exons, q


def load_fixture():
    """(genomic bytes, [chain dicts: est, exons, settings, done, dropped_first, exons_after, steps])"""
    doc = json.load(gzip.open(FIXTURE, "rt"))
    g = bytearray(RL.fixture_genomic())
    assert len(g) == doc["length"]
    for pos, s in doc["edits"]:
        g[pos:pos + len(s)] = s.encode()
    chains = []
    for est, ex, st, done, dropped, ex2, steps in doc["chains"]:
        chains.append(dict(est=est.encode(), exons=[tuple(e) for e in ex], settings=tuple(st), done=done, dropped_first=dropped,
                           exons_after=[tuple(e) for e in ex2], steps=list(steps)))
    return bytes(g), chains


# ---- today's device route: one PGPU_DP_GAP plan and one pgpu_index_refine_introns call per intron depth ---------------
def device_rounds(ctx, idx, gen, chains, clock=None):
    """chains of (est, exons, settings), every window within the caps -> [(exons afterwards, steps)]: round d aligns the
    windows of intron d of every chain that has one, cut on the host from the exons as round d - 1 left them.  `clock`
    (a dict) receives "library_s", the seconds spent inside the two library calls of every round."""
    import time
    from pintron_amd import capi
    inside = 0.0
    state = [[tuple(int(v) for v in e) for e in ex] for _, ex, _ in chains]
    steps = [[0] * len(ex) for _, ex, _ in chains]
    depth = 0
    while True:
        live = [k for k, ex in enumerate(state) if len(ex) > depth + 1]
        if not live:
            if clock is not None:
                clock["library_s"] = inside
            return list(zip(state, steps))
        jl = capi.JobList()
        for k in live:
            est, _, st = chains[k]
            se, sg = RL.gap_windows(est, gen, state[k][depth], state[k][depth + 1], *st[:3])
            jl.add(capi.GAP, se, sg)
        t0 = time.perf_counter()
        out = capi.run_jobs(ctx, jl)
        inside += time.perf_counter() - t0
        items = []
        for k, o in zip(live, out):
            assert o["status"] == 0
            est, _, st = chains[k]
            v = (o["factor_cut"], o["intron_start"], o["intron_end"], o["intron_start_on_align"], o["intron_end_on_align"])
            items.append((est, o["ea"], o["ga"], v, state[k][depth], state[k][depth + 1], depth == 0, st))
        ests, rows, q = RL.query_array(items)
        t0 = time.perf_counter()
        res = idx.refine_introns(ests, rows, q)
        inside += time.perf_counter() - t0
        for k, r in zip(live, res):
            status, refined, path, d2, a2 = RL.result_tuple(r)
            assert status == RL.OK
            state[k][depth], state[k][depth + 1] = d2, a2
            steps[k][depth + 1] = step_byte(refined, path)
        depth += 1
