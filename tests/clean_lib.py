"""CPU restatement of pgpu_index_clean_chains: what get_EST_factorizations (src/est-factorizations.c:212-244) does to one
candidate factorization before refine_intron sees it.

clean           the six steps in Python over an `ops` object that answers the three device questions (the end-exon
                alignment, the dust flags, the banded edit distance): OracleOps asks tests/oracle_lib.py; the caps of the
                entry.
einval          the PGPU_EINVAL rules of the entry for one call.
RefClean        the same steps through the six routines of the reference's object code (oracle/_ref), one forked child per
                candidate; the lists are built with list_create / list_add_to_tail and read by popping.
make_case       generated candidates: exons planted in a (mutable) seeded random sequence, with errors, Ns, lower case,
                low-complexity exons, splice sites, moved outer ends, and aimed ones for what chance rarely gives.
device_route    today's route on the device: PGPU_DP_ALIGN plans (p0 = 1 head, 2 tail) and a PGPU_DP_KBAND `tail = 1` plan,
                with the logic of clean() on the host in between.
load_fixture    tests/golden/clean_chains.json.gz (tools/make_clean_golden.py).
"""
import ctypes as C
import gzip
import json
import math
import os
import struct

import numpy as np

import oracle_lib as O
import refine_lib as RL

FIXTURE = os.path.join(RL.ROOT, "tests", "golden", "clean_chains.json.gz")
OK, ERANGE, EINVAL = 0, -34, -22
MAX_EXONS = 64            # PGPU_CLEAN_MAX_EXONS
MAX_END_EXON = 4096       # PGPU_CLEAN_MAX_END_EXON
BAND_HALF = 31            # ALIGN_BAND_HALF: align_band settles scores up to it, for lengths within it
MAX_KBAND = 31            # kband_band_sweep: 2k + 1 <= 64
GAP = 45                  # '-'
M_ENDPOINTS, M_EXTERNAL, M_DUST_GEN, M_DUST_EST, M_NOISY = 1, 2, 4, 8, 16
COVERAGE = float(np.float32(0.35))      # `coverage >= 0.35f`: the float constant, compared as a double


class Refused(Exception):
    """a cap of the entry: the query's answer is PGPU_ERANGE"""


def sub(s: bytes, a: int, b: int) -> bytes:
    """real_substring(a, b - a + 1, s): clipped at both ends of s"""
    return b"" if b < a else s[max(a, 0):b + 1]


def byte_at(s: bytes, i: int) -> int:
    return s[i] if 0 <= i < len(s) else 0


def upper(c: int) -> int:
    return c & ~32


def max_edit(n: int) -> int:
    """compute_maximum_edit_distance_for_exons (:1828-1839), in FP64"""
    rate = 0.030 if n > 100 else (0.035 if n > 50 else 0.040)
    return int(max(1.0, math.ceil(n * rate)))


class OracleOps:
    """the three questions, answered by the CPU oracle"""

    def align(self, a: bytes, b: bytes, end: int):
        return O.align(a, b)

    def dust(self, gen: bytes, est: bytes, thr: float) -> int:
        return O.dust_flags(gen, est, thr)

    def kband(self, gen: bytes, est: bytes, ub: int) -> bool:
        return bool(O.kband(gen, est, ub)["ok"])


ORACLE = OracleOps()


def end_exon_alignment(ops, a: bytes, b: bytes, end: int):
    """the alignment of an end exon (a on the EST, b on the genomic sequence) under the caps of the entry: what the plan
    builder sends to lev_wave<ALIGN> (at most 64 EST bytes) or to an align_band job that settles inside the band"""
    if len(a) > MAX_END_EXON or len(b) > MAX_END_EXON:
        raise Refused("an end exon longer than %d" % MAX_END_EXON)
    if len(a) > 64 and abs(len(a) - len(b)) > BAND_HALF:
        raise Refused("lengths further apart than the band")
    al = ops.align(a, b, end)
    if len(a) > 64 and a != b and al["score"] > BAND_HALF:
        raise Refused("the band does not settle the alignment")
    return al


def best_run(ex, bad, info):
    """update_with_subfact_with_best_coverage (:1900-1987): ex the list, bad the 1-based places of the flagged exons"""
    if not bad:
        return ex
    best = (-1, -1, -1)
    left, size, covers = 1, len(ex), []
    for right in bad:
        if left < right:
            cover = ex[right - 2][1] - ex[left - 1][0] + 1
            covers.append(cover)
            if cover > best[2]:
                best = (left, right - 1, cover)
        left = right + 1
    if left <= size:
        cover = ex[size - 1][1] - ex[left - 1][0] + 1
        covers.append(cover)
        if cover > best[2]:
            best = (left, size, cover)
    if best[0] == -1:
        return []
    if covers.count(best[2]) > 1:
        info["tie"] = True
    return ex[best[0] - 1:best[1]]


def clean(est: bytes, gen: bytes, exons, thr: float, ops=ORACLE, info=None):
    """One query -> (status, verdict, first_kept, n_kept, exons afterwards, marks).  exons: [(EST_start, EST_end,
    GEN_start, GEN_end)]; the exons afterwards are parallel to them.  `info` (a dict) receives what the fixture's cover
    counts."""
    info = {} if info is None else info
    orig = [tuple(int(v) for v in e) for e in exons]
    try:
        verdict, ex, marks = _steps(est, gen, orig, thr, ops, info)
    except Refused as why:
        info["refused"] = str(why)
        return ERANGE, 0, 0, 0, orig, [0] * len(orig)
    out = [list(e) for e in orig]
    first = n = 0
    if verdict in (0, 7):
        first, n = ex[0][4], len(ex)
        out[first][0], out[first][2] = ex[0][0], ex[0][2]
        out[first + n - 1][1], out[first + n - 1][3] = ex[-1][1], ex[-1][3]
    return OK, verdict, first, n, [tuple(e) for e in out], marks


def _steps(est, gen, orig, thr, ops, info):
    if len(orig) > MAX_EXONS:
        raise Refused("more than %d exons" % MAX_EXONS)
    ex = [list(e) + [k] for k, e in enumerate(orig)]         # [EST_start, EST_end, GEN_start, GEN_end, place in the query]
    marks = [0] * len(ex)
    # ---- step 1 (:2111-2125, :1989-2019)
    if len(ex) == 1 and (ex[0][0] < 0 or ex[0][0] >= len(est)):
        return 1, [], marks
    pe = pg = -1
    for e in ex:
        if e[0] > e[1] or e[2] > e[3] or e[0] < pe or e[2] < pg:
            return 2, [], marks
        pe, pg = e[1], e[3]
    info["single"] = len(ex) == 1
    # ---- step 2: handle_endpoints (:2127-2301)
    h = ex[0]
    a, b = sub(est, h[0], h[1]), sub(gen, h[2], h[3])
    info["band"] = len(a) > 64
    info["odd"] = any(c not in b"ACGT" for c in a)
    al = end_exon_alignment(ops, a, b, 1)
    ea, ga, dim = al["ea"], al["ga"], al["dim"]
    j = m = 0
    cf, ce = h[0], h[2]
    stop = False
    while j < dim and not stop:
        if m > 5:
            stop = True
        else:
            if ea[j] == ga[j]:
                cf += 1; ce += 1; m += 1
            else:
                if ea[j] != GAP:
                    cf += 1
                if ga[j] != GAP:
                    ce += 1
                m = 0
            j += 1
    if not stop:
        marks[h[4]] |= M_ENDPOINTS
        info["head_dropped_of_two"] = len(ex) == 2
        ex.pop(0)
    else:
        info["head_trimmed"] = (cf - m, ce - m) != (h[0], h[2])
        h[0], h[2] = cf - m, ce - m
    if not ex:
        return 3, [], marks
    t = ex[-1]
    a, b = sub(est, t[0], t[1]), sub(gen, t[2], t[3])
    info["band"] |= len(a) > 64
    info["odd"] |= any(c not in b"ACGT" for c in a)
    al = end_exon_alignment(ops, a, b, 2)
    dim = al["dim"]
    ea, ga = bytearray(al["ea"]) + b"\0\0", bytearray(al["ga"]) + b"\0\0"      # a byte behind a row reads 0
    j, m = dim - 1, 0
    cf, ce = t[1], t[3]
    stop = False
    while j >= 0 and not stop:
        if m > 10:
            stop = True
        else:
            if ea[j] == ga[j]:
                cf -= 1; ce -= 1; m += 1
            else:
                if ea[j] != GAP:
                    cf -= 1
                if ga[j] != GAP:
                    ce -= 1
                m = 0
            j -= 1
    ecl, gcl = cf + m, ce + m
    cur = j + m + 1
    stop = False
    while (ea[cur] == GAP or ga[cur] == GAP) and cur < dim - 1 and not stop:
        info["gap_closing"] = True
        row, other = (ea, ga) if ea[cur] == GAP else (ga, ea)
        tr = cur + 1
        while row[tr] == GAP:
            tr += 1
        if tr < dim and row[tr] == other[cur]:
            row[cur] = row[tr]
            row[tr] = GAP
            ecl += 1; gcl += 1
        else:
            stop = True
        cur += 1
    if gcl >= t[2]:
        info["tail_trimmed"] = (ecl, gcl) != (t[1], t[3])
        t[1], t[3] = ecl, gcl
    else:
        marks[t[4]] |= M_ENDPOINTS
        ex.pop()
    if not ex:
        return 3, [], marks
    # ---- step 3: clean_external_exons (:1706-1825)
    h = ex.pop(0)
    hl = h[3] - h[2] + 1
    ok = hl >= 10
    if ok and hl < 20:
        if upper(byte_at(gen, h[3] + 1)) != 71 or upper(byte_at(gen, h[3] + 2)) not in (84, 67):
            ok = False
        elif ex:
            nx = ex[0]
            if upper(byte_at(gen, nx[2] - 2)) != 65 or upper(byte_at(gen, nx[2] - 1)) != 71:
                ok = False
        else:
            ok = False
        if ok and sub(gen, h[2], h[3]) != sub(est, h[0], h[1]):       # the edit distance, tested `> 0`
            ok = False
    if ok:
        ex.insert(0, h)
    else:
        marks[h[4]] |= M_EXTERNAL
    if not ex:
        return 4, [], marks
    t = ex.pop()
    tl = t[3] - t[2] + 1
    ok = tl >= 10
    if ok and tl < 20:
        if upper(byte_at(gen, t[2] - 2)) != 65 or upper(byte_at(gen, t[2] - 1)) != 71:
            ok = False
        elif ex:
            pv = ex[-1]
            if upper(byte_at(gen, pv[3] + 1)) != 71 or upper(byte_at(gen, pv[3] + 2)) not in (84, 67):
                ok = False
        else:
            ok = False
        if ok and sub(gen, t[2], t[3]) != sub(est, t[0], t[1]):
            ok = False
    if ok:
        ex.append(t)
    else:
        marks[t[4]] |= M_EXTERNAL
    if not ex:
        return 4, [], marks
    # ---- step 4: clean_low_complexity_exons_2 (:1667-1704)
    bad = []
    for i, e in enumerate(ex):
        if e[2] <= e[3]:
            fl = ops.dust(sub(gen, e[2], e[3]), sub(est, e[0], e[1]), thr)
            if fl:
                marks[e[4]] |= fl << 2
                bad.append(i + 1)
    ex = best_run(ex, bad, info)
    if not ex:
        return 5, [], marks
    # ---- step 5: clean_noisy_exons (:1842-1898), only_internals = false
    if any(e[2] <= e[3] and max_edit(e[3] - e[2] + 1) > MAX_KBAND for e in ex):
        raise Refused("a bound beyond the K-band on the lanes")
    bad = []
    for i, e in enumerate(ex):
        ok = False
        if e[2] <= e[3]:
            ok = ops.kband(sub(gen, e[2], e[3]), sub(est, e[0], e[1]), max_edit(e[3] - e[2] + 1))
        if not ok:
            marks[e[4]] |= M_NOISY
            bad.append(i + 1)
    ex = best_run(ex, bad, info)
    if not ex:
        return 6, [], marks
    # ---- step 6: check_est_coverage (:2303-2321)
    cover = ex[-1][1] - ex[0][0] + 1
    return (0 if cover / len(est) >= COVERAGE else 7), ex, marks


# ---- the PGPU_EINVAL rules ------------------------------------------------------------------------------------------
def passes_step1(exons, est_len):
    if len(exons) == 1 and (exons[0][0] < 0 or exons[0][0] >= est_len):
        return False
    pe = pg = -1
    for es, ee, gs, ge in exons:
        if es > ee or gs > ge or es < pe or gs < pg:
            return False
        pe, pg = ee, ge
    return True


def einval(ests_len, gen_len, exons, queries):
    """True when pgpu_index_clean_chains refuses the whole call.  exons: array or list of 4-tuples; queries: records or
    dicts with the fields of pgpu_clean_query."""
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
        if passes_step1(mine, est_len):                    # the my_asserts of :2140-2141 and :2199-2200
            if mine[0][0] < 0 or mine[0][2] < 0 or mine[-1][1] >= est_len or mine[-1][3] >= gen_len:
                return True
    return False


# ---- the reference's object code ------------------------------------------------------------------------------------
class RefClean:
    """the six routines of the reference's object code on one genomic sequence; one forked child per candidate, for the
    routines never free a factor and a bad candidate may take the process with it"""

    def __init__(self, gen: bytes):
        L = self.L = C.CDLL(RL.REF_LIB)
        self.libc = C.CDLL(None)
        self.libc.malloc.restype = C.c_void_p
        self.libc.malloc.argtypes = [C.c_size_t]
        for n in ("list_create", "list_remove_from_head", "handle_endpoints", "clean_external_exons",
                  "clean_low_complexity_exons_2", "clean_noisy_exons"):
            getattr(L, n).restype = C.c_void_p
        L.list_add_to_tail.argtypes = [C.c_void_p, C.c_void_p]
        L.list_is_empty.restype = C.c_bool
        L.list_is_empty.argtypes = [C.c_void_p]
        L.list_remove_from_head.argtypes = [C.c_void_p]
        L.handle_endpoints.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p]
        L.clean_external_exons.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p]
        L.clean_low_complexity_exons_2.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_void_p]
        L.clean_noisy_exons.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_bool]
        L.check_est_coverage.restype = C.c_bool
        L.check_est_coverage.argtypes = [C.c_void_p, C.c_char_p]
        L.check_exon_start_end.restype = C.c_bool
        L.check_exon_start_end.argtypes = [C.c_void_p]
        L.check_for_not_source_sink_factorization.restype = C.c_bool
        L.check_for_not_source_sink_factorization.argtypes = [C.c_void_p, C.c_int]
        self.gen = gen

    def _pop_all(self, pl):
        out = []
        while not self.L.list_is_empty(pl):
            f = C.cast(self.L.list_remove_from_head(pl), C.POINTER(RL._RefFactor)).contents
            out.append((f.EST_start, f.EST_end, f.GEN_start, f.GEN_end))
        return out

    def _steps(self, est, exons, thr):
        L, gen = self.L, self.gen
        pl = L.list_create()
        for e in exons:
            p = self.libc.malloc(C.sizeof(RL._RefFactor))
            f = C.cast(p, C.POINTER(RL._RefFactor)).contents
            f.EST_start, f.EST_end, f.GEN_start, f.GEN_end = e
            L.list_add_to_tail(pl, p)
        cfg = RL._RefConfig()
        cfg.complexity_threshold = thr
        if not L.check_for_not_source_sink_factorization(pl, len(est)):
            return 1, []
        if not L.check_exon_start_end(pl):
            return 2, []
        pl = L.handle_endpoints(pl, gen, est)
        if L.list_is_empty(pl):
            return 3, []
        pl = L.clean_external_exons(pl, gen, est)
        if L.list_is_empty(pl):
            return 4, []
        pl = L.clean_low_complexity_exons_2(pl, gen, est, C.byref(cfg))
        if L.list_is_empty(pl):
            return 5, []
        pl = L.clean_noisy_exons(pl, gen, est, False)
        if L.list_is_empty(pl):
            return 6, []
        return (0 if L.check_est_coverage(pl, est) else 7), self._pop_all(pl)

    def run(self, est: bytes, exons, thr: float):
        """-> (verdict, the list as the steps left it) or None when the child dies"""
        r, w = os.pipe()
        pid = os.fork()
        if pid == 0:
            try:
                os.close(r)
                os.write(w, json.dumps(self._steps(est, exons, thr)).encode())
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
        verdict, ex = json.loads(data)
        return verdict, [tuple(e) for e in ex]


def kept_list(answer):
    """the list the steps left, as RefClean.run gives it, from an answer of clean()"""
    status, verdict, first, n, ex2, marks = answer
    return verdict, [tuple(e) for e in ex2[first:first + n]]


# ---- generated inputs -----------------------------------------------------------------------------------------------
# dustScore of a random exon is about 0.3, of (CA)n 2.5, of poly-A just below 5
THRESHOLDS = (20.0, 4.0, 2.0, 1.0, 0.32)
AIMS = (None, None, None, None, None, None, "v1", "lowc", "tie", "tailgap", "drop-head2", "flank", "v3", "noisy")
_ACGT = np.frombuffer(b"ACGT", np.uint8)


def mutate(rng, s, rate):
    out = bytearray()
    for c in s:
        r = rng.random()
        if r < rate / 3:
            continue
        if r < 2 * rate / 3:
            out.append(int(_ACGT[rng.integers(4)]))
            out.append(c)
            continue
        if r < rate:
            out.append(int(_ACGT[rng.integers(4)]))
            continue
        out.append(c)
    return out


def make_case(rng, gen: bytearray, pos, aim=None, k=0):
    """plants a candidate at `pos` of the (mutable) sequence -> (est, exons, threshold, end): one to six exons of 8 to 400
    bases with 0 to 30 % errors (the higher rates on the short exons: the band has to settle the long ones), Ns, lower
    case, low-complexity exons, splice sites, flanks on the EST and outer ends moved by a few bases.  Aims: `v1` one exon
    that begins outside the EST, `lowc` every exon of low complexity, `tie` two equal runs around a flagged exon,
    `tailgap` a base missing a few columns inside the tail, `drop-head2` two exons whose head matches nowhere, `v3` one
    exon that matches nowhere, `noisy` every exon with 8 % errors, `flank` long unaligned ends of the EST."""
    n = int(rng.integers(1, 7))
    if aim in ("v1", "v3"):
        n = 1
    elif aim == "tie":
        n = 3
    elif aim == "drop-head2":
        n = 2
    p = pos + int(rng.integers(2, 60))
    est, exons = bytearray(), []
    if rng.random() < 0.3 or aim == "flank":
        est += RL.rnd(rng, int(rng.integers(150, 400)) if aim == "flank" else int(rng.integers(1, 60)))
    tie_len = int(rng.integers(30, 90))
    for i in range(n):
        kind = int(rng.integers(10))
        ln = int(rng.integers(8, 24)) if kind < 3 else (int(rng.integers(160, 400)) if kind == 9 else int(rng.integers(25, 160)))
        if aim in ("lowc", "tailgap"):
            ln = max(ln, 30)
        if aim == "tie":
            ln, kind = (tie_len, 5) if i != 1 else (int(rng.integers(30, 60)), 3)
        if aim == "noisy":
            ln = int(rng.integers(60, 160))
        unmatched = (aim == "drop-head2" and i == 0) or aim == "v3"
        if unmatched:
            ln = int(rng.integers(20, 56))                # within what lev_wave<ALIGN> takes, whatever the score
        if kind == 3 or aim == "lowc":
            gen[p:p + ln] = (b"CA" * ln)[:ln] if rng.random() < .5 else b"A" * ln
        if rng.random() < 0.7:
            gen[p + ln:p + ln + 2] = b"GT" if rng.random() < .8 else b"gc"
        piece = bytes(gen[p:p + ln])
        rate = (0.0, 0.0, 0.01, 0.03, 0.05, 0.10, 0.3)[int(rng.integers(7 if ln <= 55 else 5))]
        if aim == "tie":
            rate = 0.0
        if aim == "noisy":
            rate = 0.08
        e = mutate(rng, piece, rate)
        if unmatched:
            e = bytearray(RL.rnd(rng, ln))
        if aim == "tailgap" and i == n - 1:
            cut = len(e) - int(rng.integers(3, 10))
            e = e[:cut] + e[cut + 1:] if rng.random() < 0.5 else e[:cut] + e[cut - 1:cut] + e[cut:]
        if aim != "tie":
            if rng.random() < 0.1 and len(e) > 3:
                e[int(rng.integers(len(e)))] = 78
            if rng.random() < 0.05:
                e = bytearray(bytes(e).lower())
        if not e:
            e = bytearray(b"A")
        exons.append((len(est), len(est) + len(e) - 1, p, p + ln - 1))
        est += e
        p += ln + int(rng.integers(60, 200))
        if rng.random() < 0.7:
            gen[p - 2:p] = b"AG" if rng.random() < .85 else b"ag"
    if rng.random() < 0.3 or aim == "flank":
        est += RL.rnd(rng, int(rng.integers(150, 400)) if aim == "flank" else int(rng.integers(1, 80)))
    if aim not in ("tie", "tailgap"):                    # the outer ends, moved
        if rng.random() < 0.5:
            e = exons[0]
            d = int(rng.integers(0, 12))
            exons[0] = (max(0, e[0] - d), e[1], max(0, e[2] - d), e[3])
        if rng.random() < 0.5:
            e = exons[-1]
            d = int(rng.integers(0, 15))
            exons[-1] = (e[0], min(len(est) - 1, e[1] + d), min(e[2], len(gen) - 1), min(len(gen) - 1, e[3] + d))
        if rng.random() < 0.03:
            j = int(rng.integers(n))
            exons[j] = (exons[0][1], exons[0][0] - 1, exons[0][2], exons[0][3])
    if aim == "v1":
        e = exons[0]
        exons[0] = (-1, e[1], e[2], e[3]) if rng.random() < 0.5 else (len(est), len(est), e[2], e[3])
    return bytes(est), exons, 2.0 if aim in ("lowc", "tie") else THRESHOLDS[k % len(THRESHOLDS)], p


def batch_arrays(cases):
    """cases of (est, exons, threshold) -> (ests, exons array, queries array) in the layouts of the entry; equal ESTs are
    stored once"""
    from pintron_amd import capi
    n_ex = sum(len(c[1]) for c in cases)
    exons = np.zeros(n_ex, dtype=np.dtype(capi.FACTOR_DTYPE))
    q = np.zeros(len(cases), dtype=np.dtype(capi.CLEAN_QUERY_DTYPE))
    ests, eat, eoff, k = [], {}, 0, 0
    for i, (est, ex, thr) in enumerate(cases):
        if est not in eat:
            eat[est] = eoff
            ests.append(est)
            eoff += len(est)
        for e in ex:
            exons[k] = tuple(e)
            k += 1
        q[i] = (eat[est], len(est), k - len(ex), len(ex), 0, thr)
    return b"".join(ests), exons, q


def expect_arrays(exons, answers):
    """answers of clean() per query, in the order of the exons -> the three arrays of the entry"""
    from pintron_amd import capi
    out_exons = exons.copy()
    out_marks = np.zeros(len(exons), dtype=np.uint8)
    res = np.zeros(len(answers), dtype=np.dtype(capi.CLEAN_RESULT_DTYPE))
    k = 0
    for i, (status, verdict, first, n, ex2, marks) in enumerate(answers):
        res[i] = (status, verdict, first, n)
        for e, m in zip(ex2, marks):
            out_exons[k] = tuple(e)
            out_marks[k] = m
            k += 1
    assert k == len(exons)
    return out_exons, out_marks, res


def load_fixture():
    """(genomic bytes, [case dicts: est, exons, thr, verdict, first, n, exons_after, marks, tags])"""
    doc = json.load(gzip.open(FIXTURE, "rt"))
    g = bytearray(RL.rnd(np.random.default_rng(doc["seed"]), doc["length"]))
    for pos, s in doc["edits"]:
        g[pos:pos + len(s)] = s.encode()
    cases = []
    for est, ex, thr, verdict, first, n, ends, marks, tags in doc["cases"]:
        ex = [tuple(e) for e in ex]
        after = [list(e) for e in ex]
        if n:
            after[first][0], after[first][2], after[first + n - 1][1], after[first + n - 1][3] = ends
        cases.append(dict(est=est.encode(), exons=ex, thr=thr, verdict=verdict, first=first, n=n,
                          exons_after=[tuple(e) for e in after], marks=list(marks), tags=set(tags)))
    return bytes(g), cases


TAGS = ("head_trimmed", "gap_closing", "single", "head_dropped_of_two", "tie", "band", "odd")


def tags_of(info):
    return sorted(t for t in TAGS if info.get(t)) + (["tail_trimmed_gap"] if info.get("tail_trimmed") and info.get("gap_closing") else [])


# ---- today's device route ---------------------------------------------------------------------------------------------
class _Need(Exception):
    pass


class _DeviceOps:
    """answers from the plans run so far; a question without an answer is noted for the next plan"""

    def __init__(self):
        self.aligned, self.checked = {}, {}
        self.want_align, self.want_check = {}, {}
        self.missing = False

    def align(self, a, b, end):
        got = self.aligned.get((a, b))
        if got is None:
            self.want_align[(a, b)] = end
            raise _Need()
        return got

    def _check(self, gen, est, thr):
        got = self.checked.get((gen, est, thr))
        if got is None:
            self.want_check[(gen, est, thr)] = True
            self.missing = True
            return 0, False
        return got

    def dust(self, gen, est, thr):
        self.thr = thr
        return self._check(gen, est, thr)[0]

    def kband(self, gen, est, ub):
        assert ub == max_edit(len(gen))
        return self._check(gen, est, self.thr)[1]


def run_plan_timed(ctx, jl):
    """capi.run_jobs with a clock around the library's own entry points alone: pgpu_dp_plan_create, _launch, _sync, _fetch
    and _destroy.  The job table and the arena are packed before it starts and the results are decoded after it stops
    -> (decoded results, seconds inside the library)"""
    import time
    from pintron_amd import capi
    L = ctx.L
    jobs, arena = jl.arrays()
    n = len(jl.jobs)
    res = (capi.DpResult * max(n, 1))()
    h = C.c_void_p()
    t0 = time.perf_counter()
    rc = L.pgpu_dp_plan_create(ctx.h, None, jobs, n, arena, len(arena), C.byref(h))
    inside = time.perf_counter() - t0
    ctx.check(rc)
    try:
        t0 = time.perf_counter()
        rc = L.pgpu_dp_plan_launch(ctx.h, h) or L.pgpu_dp_plan_sync(ctx.h, h)
        nbytes = L.pgpu_dp_plan_string_bytes(h)
        inside += time.perf_counter() - t0
        ctx.check(rc)
        sbuf = C.create_string_buffer(max(nbytes, 1))
        t0 = time.perf_counter()
        rc = L.pgpu_dp_plan_fetch(ctx.h, h, res, sbuf, nbytes)
        inside += time.perf_counter() - t0
        ctx.check(rc)
    finally:
        t0 = time.perf_counter()
        L.pgpu_dp_plan_destroy(ctx.h, h)
        inside += time.perf_counter() - t0
    strings = sbuf.raw
    return [capi.decode(jl.jobs[i].kind, res[i], strings) for i in range(n)], inside


def device_route(ctx, gen: bytes, cases, clock=None):
    """cases of (est, exons, threshold) -> the answers of clean(), every question asked of the device: rounds of one
    PGPU_DP_ALIGN plan (p0 = 1 for a head, 2 for a tail) or one PGPU_DP_KBAND `tail = 1` plan (p1 / p2 the threshold) over
    what the cases ask next.  `clock` (a dict) receives "library_s", the seconds inside the library's entry points
    (run_plan_timed: packing the jobs and decoding the answers in Python are outside it), "plans" and "jobs"."""
    from pintron_amd import capi
    ops = _DeviceOps()
    answers = [None] * len(cases)
    inside, plans, n_jobs = 0.0, 0, 0
    while True:
        ops.want_align, ops.want_check = {}, {}
        for k, (est, ex, thr) in enumerate(cases):
            if answers[k] is not None:
                continue
            ops.missing = False
            try:
                got = clean(est, gen, ex, thr, ops=ops)
            except _Need:
                continue
            if not ops.missing:
                answers[k] = got
        if not ops.want_align and not ops.want_check:
            break
        jl = capi.JobList()
        keys = []
        for (a, b), end in ops.want_align.items():
            jl.add(capi.ALIGN, a, b, p0=end)
            keys.append(("a", (a, b)))
        for (g, e, thr) in ops.want_check:
            lo, hi = struct.unpack("<II", struct.pack("<d", thr))
            jl.add(capi.KBAND, g, e, p0=max_edit(len(g)), p1=lo, p2=hi, tail=1)
            keys.append(("c", (g, e, thr)))
        out, spent = run_plan_timed(ctx, jl)
        inside, plans, n_jobs = inside + spent, plans + 1, n_jobs + len(keys)
        for (what, key), o in zip(keys, out):
            assert o["status"] == 0, o
            if what == "a":
                ops.aligned[key] = o
            else:
                ops.checked[key] = (o["dust"], bool(o["ok"]))
    if clock is not None:
        clock["library_s"], clock["plans"], clock["jobs"] = inside, plans, n_jobs
    assert all(a is not None for a in answers)
    return answers
