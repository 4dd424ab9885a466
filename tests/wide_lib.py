"""The wide entries -- pgpu_index_tail_chains_wide, pgpu_index_small_chains_wide and the two wide final forms
(include/pintron_gpu.h) -- restated, and their hand-made cases.

The restatements are the ones of tests/tail_lib.py, tests/small_lib.py and tests/final_lib.py, run with the two caps the wide
kernels lift (tail_lib.MAX_AFFIX, small_lib.MAX_PREFIX_WINDOW: module globals read at call time) set to the wide values
for the duration of the call and restored afterwards.  Everything else of the three libraries is as it is.

The cases are lost prefix and suffix windows, and prefix windows of the small stage, at the lengths where something
changes: the narrow cap (256), the first wide length (257), a lane boundary at 16 rows per lane (271-273), the cap of 8
rows per lane (511-513), the wide cap (1023, 1024) and one past it (1025).  All of them lie over ONE seeded sequence; the
fixture (tests/golden/wide_chains.json.gz, tools/make_wide_golden.py) stores them with their answers."""
import contextlib
import gzip
import json
import os
import types

import numpy as np

import refine_lib as RL
import small_lib as SL
import tail_lib as TL

FIXTURE = os.path.join(RL.ROOT, "tests", "golden", "wide_chains.json.gz")

TAIL_WIDE_MAX_AFFIX = 1024            # PGPU_TAIL_WIDE_MAX_AFFIX
SMALL_WIDE_MAX_PREFIX_WINDOW = 1024   # PGPU_SMALL_WIDE_MAX_PREFIX_WINDOW
WIDE_AFFIX_GEN = int(1.17 * 1024)     # 1198: the genomic window of the widest prefix
NARROW_MAX_AFFIX = 256                # PGPU_TAIL_MAX_AFFIX and PGPU_SMALL_MAX_PREFIX_WINDOW, whatever the libraries' globals hold
NARROW_MAX_PREFIX_WINDOW = 256        # at the time of a call

WIDTHS = (256, 257, 271, 272, 273, 511, 512, 513, 1023, 1024, 1025)
MIN_PER_TAG = 10
MIL = 40

TAIL_TAGS = tuple("affix_%d" % w for w in WIDTHS) + (
    "pre_wide", "suf_wide", "wide_recovered", "wide_no_cut", "wide_skipped", "both_wide", "gen_1198", "gen_clipped", "gs_below_es",
    "tail_other_cap")
SMALL_TAGS = tuple("window_%d" % w for w in WIDTHS) + ("wide_inserted", "wide_not_inserted", "tail_wide_too", "small_other_cap")
TAGS = TAIL_TAGS + SMALL_TAGS


# ---- the wide restatements --------------------------------------------------------------------------------------------
@contextlib.contextmanager
def caps(affix=TAIL_WIDE_MAX_AFFIX, window=SMALL_WIDE_MAX_PREFIX_WINDOW):
    """the two caps of the restatements at other values, for the calls inside"""
    old = TL.MAX_AFFIX, SL.MAX_PREFIX_WINDOW
    TL.MAX_AFFIX, SL.MAX_PREFIX_WINDOW = affix, window
    try:
        yield
    finally:
        TL.MAX_AFFIX, SL.MAX_PREFIX_WINDOW = old


def tail(*args, **kw):
    """tail_lib.tail with a lost window of up to 1024 EST bytes"""
    with caps():
        return TL.tail(*args, **kw)


def small(*args, **kw):
    """small_lib.small with a prefix window of up to 1024 EST bytes"""
    with caps():
        return SL.small(*args, **kw)


def final(*args, **kw):
    """final_lib.final over the two wide stages"""
    import final_lib as FL
    with caps():
        return FL.final(*args, **kw)


class Cut304Ops:
    """tail_lib's oracle with the genomic window of a lost prefix cut at 304 bytes, the narrow kernel's LDS: a broken
    restatement the fixture must notice (a prefix is the one question whose genomic window is the longer one)"""

    def __getattr__(self, name):
        return getattr(TL.ORACLE, name)

    def affix(self, e, g):
        return TL.ORACLE.affix(e, g[:304] if len(g) > len(e) else g)


# ---- the tags ---------------------------------------------------------------------------------------------------------
def tail_windows(est: bytes, gen: bytes, exons):
    """((EST bytes, genomic bytes, asked) of the lost prefix, the same of the lost suffix) as step 4 takes them from the
    exons as step 1 left them; (0, 0, False) where there is no window"""
    ex = [list(e) for e in exons]
    TL.correct_tail(est, gen, ex[-1])
    ff, fl = ex[0], ex[-1]
    pre = suf = (0, 0, False)
    if ff[0] > 0 and ff[2] > 0:
        cap = int((1.0 + TL.MAX_ERROR_RATE) * min(ff[0], ff[2]))
        pre = (min(ff[0], cap), min(ff[2], cap), est[ff[0] - 1] != gen[ff[2] - 1])
    if len(est) - fl[1] > 1 and len(gen) - fl[3] > 1:
        n = min(len(est) - fl[1] - 1, len(gen) - fl[3] - 1)
        suf = (n, n, est[fl[1]] != gen[fl[3]])
    return pre, suf


def tail_tags(orig: bytes, est: bytes, gen: bytes, exons, answer, info):
    """the TAIL_TAGS a case shows: `answer` and `info` of the wide restatement"""
    tags = set()
    if orig != est:
        return tags
    pre, suf = tail_windows(est, gen, exons)
    wide = [w[0] > NARROW_MAX_AFFIX for w in (pre, suf)]
    for w in (pre, suf):
        if w[0] in WIDTHS:
            tags.add("affix_%d" % w[0])
    if wide[0] and pre[2]:
        tags.add("pre_wide")
    if wide[1] and suf[2]:
        tags.add("suf_wide")
    if wide[0] and pre[2] and wide[1] and suf[2]:
        tags.add("both_wide")
    if (wide[0] and not pre[2]) or (wide[1] and not suf[2]):
        tags.add("wide_skipped")
    if answer[0] == TL.OK and ((wide[0] and answer[4] & 1) or (wide[1] and answer[4] & 2)):
        tags.add("wide_recovered")
    if answer[0] == TL.OK and ((wide[0] and pre[2] and info.get("pre_no_cut")) or (wide[1] and suf[2] and info.get("suf_no_cut"))):
        tags.add("wide_no_cut")
    if pre[2] and pre[1] == WIDE_AFFIX_GEN:
        tags.add("gen_1198")
    if wide[0] and pre[2] and pre[0] == exons[0][0] and pre[1] == exons[0][2] < int(1.17 * pre[0]):
        tags.add("gen_clipped")
    if wide[0] and pre[2] and exons[0][2] < exons[0][0]:
        tags.add("gs_below_es")
    if answer[0] != TL.OK and max(pre[0] if pre[2] else 0, suf[0] if suf[2] else 0) in range(NARROW_MAX_AFFIX + 1, TAIL_WIDE_MAX_AFFIX + 1):
        tags.add("tail_other_cap")
    return tags


def small_tags(est: bytes, gen: bytes, exons, answer, info):
    """the SMALL_TAGS a case shows: `answer` and `info` of the wide restatement, info["allelen"] what step 1 reached"""
    tags = set()
    w = info.get("allelen", 0)
    if w in WIDTHS:
        tags.add("window_%d" % w)
    if NARROW_MAX_PREFIX_WINDOW < w <= SMALL_WIDE_MAX_PREFIX_WINDOW:
        if answer[0] == SL.OK:
            tags.add("wide_inserted" if answer[3] else "wide_not_inserted")
        else:
            tags.add("small_other_cap")
        pre = tail_windows(est, gen, exons)[0]
        if pre[0] > NARROW_MAX_AFFIX and pre[2]:
            tags.add("tail_wide_too")
    return tags


class _AllelenOps:
    """small_lib's oracle, noting the pattern length of the one border refinement step 1 asks"""

    def __init__(self, ops, info):
        self._ops, self._info = ops, info

    def __getattr__(self, name):
        return getattr(self._ops, name)

    def borders(self, p, *rest):
        self._info["allelen"] = len(p)
        return self._ops.borders(p, *rest)


def small_allelen(orig, est, gen, exons, mil, ops):
    """the allelen at which step 1 reaches its border refinement, caps lifted (0: it does not)"""
    seen = {}
    SL.small(orig, est, gen, exons, mil, ops=_AllelenOps(ops, seen), info={"no_caps": True})
    return seen.get("allelen", 0)


# ---- the hand-made cases ----------------------------------------------------------------------------------------------
GEN_LEN = 200_000
HEAD = 3_000              # read only, and the place of the cases that need an exon near the sequence's start
WRITE_END = 110_000       # builders that write into the sequence take slots in [HEAD, WRITE_END); behind it: read only
SEED = 1021


class World:
    """the sequence under construction and the cases planted in it: tail cases (name, orig, est, exons), small cases
    (name, orig, est, exons, min_intron_length)"""

    def __init__(self, seed=SEED):
        self.seed = seed
        self.rng = np.random.default_rng(seed)
        self.g = bytearray(RL.rnd(self.rng, GEN_LEN))
        self.next_free = HEAD
        self.tail_cases, self.small_cases = [], []

    def slot(self, size):
        at = self.next_free
        self.next_free += size
        assert self.next_free <= WRITE_END
        return at

    def spot(self, room=3000, lead=1400):
        return int(self.rng.integers(WRITE_END + lead, GEN_LEN - room))

    def add_tail(self, name, est, exons):
        est = bytes(est)
        self.tail_cases.append((name, est, est, [tuple(int(v) for v in e) for e in exons]))

    def add_small(self, name, est, exons, mil=MIL):
        est = bytes(est)
        self.small_cases.append((name, est, est, [tuple(int(v) for v in e) for e in exons], int(mil)))


def _ending(w, end):
    """behind the last exon: a byte that differs from the sequence (step 1 adds nothing) and two more"""
    return bytes([TL.other_base(w.g[end])]) + RL.rnd(w.rng, 2)


def _prefix_flank(w, at, width, kind):
    """the whole EST in front of a first exon at g[at]: a copy of the sequence there with the byte beside the exon
    substituted (recovered), unrelated bytes (no_cut), or the copy as it is (skipped: equal first bytes, no DP)"""
    g = w.g
    lo = max(0, at - width)
    flank = bytearray(RL.rnd(w.rng, width - (at - lo)) + bytes(g[lo:at])) if kind != "no_cut" else bytearray(RL.rnd(w.rng, width))
    if kind == "skipped":
        flank[-1] = g[at - 1]
    else:
        flank[-1] = TL.other_base(g[at - 1])
    return bytes(flank)


def _suffix_body(w, end, width, kind):
    """what follows a last exon that ends at g[end - 1], `width` bytes: the window starts ON the exon's last byte.  Its
    first byte differs from the sequence so that step 1 adds nothing; then a copy of the sequence (recovered, skipped) or
    unrelated bytes (no_cut)"""
    g = w.g
    body = bytearray(g[end:end + width]) if kind != "no_cut" else bytearray(RL.rnd(w.rng, width))
    body[0] = TL.other_base(g[end])
    return body


def build_tail_cases(w, reps=2):
    rng, g = w.rng, w.g
    for rep in range(reps):
        for width in WIDTHS:
            for kind in ("recovered", "no_cut", "skipped"):
                # a lost prefix
                at = w.spot()
                est, ex, end = TL.chain(g, at, TL._plain(w, int(rng.integers(1, 4))), flank=_prefix_flank(w, at, width, kind))
                w.add_tail("pre_%d_%s" % (width, kind), est + _ending(w, end), ex)
                # a lost suffix: the EST has `width` bytes behind the exon
                at = w.spot()
                est, ex, end = TL.chain(g, at, TL._plain(w, int(rng.integers(1, 4))))
                if kind != "skipped":
                    est[-1] = TL.other_base(est[-1])
                w.add_tail("suf_%d_%s" % (width, kind), est + _suffix_body(w, end, width, kind), ex)
    for rep in range(MIN_PER_TAG):
        # both windows wide in one query
        wp, ws = [int(rng.integers(257, 1025)) for _ in range(2)]
        at = w.spot()
        est, ex, end = TL.chain(g, at, TL._plain(w, int(rng.integers(1, 4))), flank=_prefix_flank(w, at, wp, "recovered"))
        est[-1] = TL.other_base(est[-1])
        w.add_tail("both_%d_%d" % (wp, ws), est + _suffix_body(w, end, ws, "recovered" if rep % 2 else "no_cut"), ex)
        # the genomic window at its largest: 1 024 EST bytes against (int)(1.17 * 1024) = 1 198 of the sequence
        at = w.spot()
        est, ex, end = TL.chain(g, at, TL._plain(w, 2), flank=_prefix_flank(w, at, 1024, "no_cut" if rep % 2 else "recovered"))
        w.add_tail("gen_1198", est + _ending(w, end), ex)
        # the genomic window clipped by GEN_start: an exon 1 024 .. 1 197 bytes into the sequence behind 1 024 EST bytes
        at = int(rng.integers(1024, WIDE_AFFIX_GEN))
        est, ex, end = TL.chain(g, at, TL._plain(w, 2), flank=_prefix_flank(w, at, 1024, "recovered" if rep % 2 else "no_cut"))
        w.add_tail("clipped_%d" % at, est + _ending(w, end), ex)
        # GEN_start below EST_start: the window is 1.17 x GEN_start on the EST, GEN_start on the sequence
        at = int(rng.integers(300, 800))
        est, ex, end = TL.chain(g, at, TL._plain(w, 2), flank=_prefix_flank(w, at, at + int(rng.integers(150, 400)), "recovered"))
        w.add_tail("gs_below_es_%d" % at, est + _ending(w, end), ex)
        # refused at 257 by the narrow cap, and by step 5's window of 129 in the wide kernel
        at = w.slot(1100)
        k = int(rng.integers(0, 20))
        quiet = types.SimpleNamespace(rng=rng, g=g)
        body, ex = TL._false_small(quiet, at + 400, (150, 150, 30), (b"CC", b"CC", b"CC", b"CC"), 100, gap=(RL.rnd(rng, k), RL.rnd(rng, 19 - k)))
        width = int(rng.integers(257, 400))
        flank = _prefix_flank(w, at + 400, width, "recovered")
        ex = [(a + width, b + width, c, d) for a, b, c, d in ex]
        w.add_tail("other_cap_window_129", flank + body + _ending(w, ex[-1][3] + 1), ex)


def _small_locus(w, s_len, a_len=60, intron=90):
    """[S][GT .. AG][A] in a slot of its own -> (start of S, start of A)"""
    at = w.slot(s_len + intron + a_len + 40) + 20
    a0 = at + s_len + intron
    w.g[at + s_len:at + s_len + 2] = b"GT"
    w.g[a0 - 2:a0] = b"AG"
    return at, a0


def build_small_cases(w, reps=5):
    rng, g = w.rng, w.g
    a_len = 60
    for rep in range(reps):
        for allelen in WIDTHS:
            # without the inserted exon: the factor (20 bytes in front of an intron) at the first byte of the piece, whose
            # offset is then misused as an EST coordinate; in front of it unrelated bytes: the refinement finds no cut
            s0, a0 = _small_locus(w, 20)
            start = allelen - 23
            est = RL.rnd(rng, start - 46) + bytes(g[s0:s0 + 20]) + RL.rnd(rng, 26) + bytes(g[a0:a0 + a_len])
            w.add_small("window_%d_plain" % allelen, est, [(start, start + a_len - 1, a0, a0 + a_len - 1)])
            # with it: a lost exon X = V + V[:46] of allelen - 23 bytes in front of A.  The last 46 bytes of X are its first
            # ones, so the longest factor of the piece is found at X's first byte, pe = 0, and the pattern is X + A[:23]
            n = allelen - 23
            s0, a0 = _small_locus(w, n)
            v = RL.rnd(rng, n - 46)
            g[s0:s0 + n] = v + v[:46]
            est = bytes(g[s0:s0 + n]) + bytes(g[a0:a0 + a_len])
            w.add_small("window_%d_inserted" % allelen, est, [(n, n + a_len - 1, a0, a0 + a_len - 1)])
    for rep in range(MIN_PER_TAG):
        # refused at 257 by the narrow cap, and by the K-band of 32 in the wide kernel: a second exon of 1 034 genomic bytes
        allelen = int(rng.integers(257, 600))
        s0, a0 = _small_locus(w, 20)
        b0 = w.slot(1034 + 200) + 150
        start = allelen - 23
        est = RL.rnd(rng, start - 46) + bytes(g[s0:s0 + 20]) + RL.rnd(rng, 26) + bytes(g[a0:a0 + a_len])
        e0 = len(est)
        est += bytes(g[b0:b0 + 1034])
        w.add_small("other_cap_kband_32", est, [(start, start + a_len - 1, a0, a0 + a_len - 1), (e0, e0 + 1033, b0, b0 + 1033)])


def ordinary(w, n=3):
    """([tail cases], [small cases]) that no cap concerns, as neighbours in a batch: read only"""
    rng, g = w.rng, w.g
    tails, smalls = [], []
    for _ in range(n):
        at = w.spot()
        k = int(rng.integers(8, 40))
        flank = bytes(g[at - k:at - 1]) + bytes([TL.other_base(g[at - 1])])
        est, ex, end = TL.chain(g, at, TL._plain(w, 3), flank=flank)
        est = bytes(est + _ending(w, end))
        tails.append(("ordinary", est, est, [tuple(e) for e in ex]))
        at = w.spot()
        est, ex, end = TL.chain(g, at, TL._plain(w, 3, lens=(30, 90)))
        smalls.append(("ordinary", bytes(est), bytes(est), [tuple(e) for e in ex], MIL))
    return tails, smalls


_world = []


def make_world(seed=SEED):
    """(the sequence, tail cases, small cases, (ordinary tail cases, ordinary small cases)); computed once"""
    if not _world:
        w = World(seed)
        build_small_cases(w)
        build_tail_cases(w)
        neighbours = ordinary(w)
        _world.append((bytes(w.g), w.tail_cases, w.small_cases, neighbours))
    return _world[0]


# ---- the fixture ------------------------------------------------------------------------------------------------------
_fixture = []


def load_fixture():
    """(sequence, [tail case dicts: name, orig, est, exons, answer, tags], [small case dicts: ... mil ...])"""
    if not _fixture:
        doc = json.load(gzip.open(FIXTURE, "rt"))
        g = bytearray(RL.rnd(np.random.default_rng(doc["seed"]), doc["length"]))
        for pos, s in doc["edits"]:
            g[pos:pos + len(s)] = s.encode()
        _fixture.append((bytes(g), TL._case_dicts(doc["tail"]), SL._case_dicts(doc["small"])))
    return _fixture[0]
