#!/usr/bin/env python3
"""Writes tests/golden/small_chains.json.gz and small_chains.md: what the last two routines of refine_EST_factorizations
(search_for_new_small_exons, clean_factorizations) make of one factorization, on hand-made factorizations over seeded
sequences (tests/small_lib.py: one builder per group of tags of the cover) and on the factorizations of c2, test-AMBN and
test-issue-13 as the tail fixture (tests/golden/tail_chains.json.gz) left them.

A case is stored only when three witnesses agree; a disagreement ends the run, and no case is dropped.
  1. The reference's own object code, refine_EST_factorizations of oracle/_ref/libpintron_ref_core.so (made by build()
     where the reference's sources are), static helpers included, on lists built with its own list_create /
     list_add_to_tail / factor_create, in a child process.  It is held against the composition on the same input: steps 3 to
     5 of tests/tail_lib.py (remove_invalid, recover_affixes, remove_false_small_exons) and then the new restatement on
     what they keep, both with the caps lifted.
  2. The restatement alone, tests/small_lib.py, over the CPU oracle: its answer is what is stored.
  3. The host's own routines, ef_chain_small of tests/hostcheck/libestfact_check.so, over the oracle as backend.
A case in which the reference would read outside a string or ends the program on an assertion (a splice-site test that
leaves the sequence, an exon shorter than a perfect border, a list that is not in order) is tagged `outside` or
`disordered` and carries witnesses 2 and 3, or 2 alone where the host code makes the same read; so does a case the
reference's process does not survive.  A case beyond a cap of the entry is stored with its refusal; the reference and the
host code have no caps, so they are held against the restatement with the caps lifted.

Before writing, the tool breaks the restatement three ways -- an inserted exon is analysed again, step 3 runs on the
working sequence, step 3 runs in clean_chains' order -- and checks that answers of the hand-made cases change each time: a
fixture that one of those wrong builds would pass is not written.

The file holds data only.  It is not written unless it holds the cover tests/small_lib.py asks for.

    python tools/make_small_golden.py
"""
import ctypes as C
import gzip
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle_lib as O  # noqa: E402
import refine_lib as RL  # noqa: E402
import small_lib as SL  # noqa: E402
import tail_lib as TL  # noqa: E402

SEED = 907
LIMIT = 1 << 20
REAL_MIL = 40             # config->min_intron_length of the real inputs' runs (the default)


class _Node(C.Structure):
    pass


_Node._fields_ = [("next", C.POINTER(_Node)), ("prev", C.POINTER(_Node)), ("element", C.c_void_p)]


class _List(C.Structure):            # include/list.h: struct _list
    _fields_ = [("sentinel", C.POINTER(_Node)), ("size", C.c_size_t)]


def _elements(lst):
    l = C.cast(lst, C.POINTER(_List)).contents
    out, node = [], l.sentinel.contents.next
    for _ in range(l.size):
        out.append(node.contents.element)
        node = node.contents.next
    return out


class Ref:
    """refine_EST_factorizations of the reference's object code, on its own lists, in a child process"""

    def __init__(self, gen: bytes):
        R = self.R = O.ref()
        R.list_create.restype = C.c_void_p
        R.list_add_to_tail.argtypes = [C.c_void_p, C.c_void_p]
        R.factor_create.restype = C.c_void_p
        R.refine_EST_factorizations.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        self.gen = C.create_string_buffer(gen)
        self.gi = (C.c_void_p * 32)()                        # struct _EST_info: original_EST_seq, EST_seq, ...
        self.gi[0] = self.gi[1] = C.addressof(self.gen)

    def _refine(self, orig, est, exons, mil):
        R = self.R
        lst = R.list_create()
        for e in exons:
            f = R.factor_create()
            C.cast(f, C.POINTER(RL._RefFactor)).contents.__init__(*e)
            R.list_add_to_tail(lst, f)
        outer = R.list_create()
        R.list_add_to_tail(outer, lst)
        ob, eb = C.create_string_buffer(orig), C.create_string_buffer(est)
        ei = (C.c_void_p * 32)()
        ei[0], ei[1] = C.addressof(ob), C.addressof(eb)
        pest = (C.c_void_p * 16)()                           # struct _EST: info, factorizations, ...
        pest[0], pest[1] = C.addressof(ei), outer
        cfg = RL._RefConfig()
        cfg.min_intron_length = mil
        R.refine_EST_factorizations(C.addressof(self.gi), C.addressof(pest), C.byref(cfg))
        facts = _elements(pest[1])
        if not facts:
            return []
        out = []
        for f in _elements(facts[0]):
            x = C.cast(f, C.POINTER(RL._RefFactor)).contents
            out.append([x.EST_start, x.EST_end, x.GEN_start, x.GEN_end])
        return out

    def refine(self, orig, est, exons, mil):
        """the exons refine_EST_factorizations leaves ([] when none), or None when the child does not survive the call"""
        r, w = os.pipe()
        pid = os.fork()
        if pid == 0:
            try:
                os.close(r)
                devnull = os.open(os.devnull, os.O_WRONLY)
                os.dup2(devnull, 1)
                os.dup2(devnull, 2)
                os.write(w, json.dumps(self._refine(orig, est, exons, mil)).encode())
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
        return [tuple(e) for e in json.loads(data)]


def composition(orig, est, gen, exons, mil, ops):
    """steps 3-5 of tests/tail_lib.py, then the new restatement on what they keep, caps lifted -> (the exons left, or None
    where the composition has no answer the reference could give: a list out of order, a read outside a string)"""
    ex = [list(e) for e in exons]
    steps = [0] * len(ex)
    info = {"no_caps": True}
    if TL.invalid(ex, info):
        return []
    TL.recover_affixes(est, gen, ex, steps, TL.ORACLE, info)
    TL.remove_false_small_exons(est, gen, ex, steps, TL.ORACLE, info)
    kept = [tuple(e) for e, s in zip(ex, steps) if s & 3 != TL.REMOVED]
    info2 = {"no_caps": True}
    a = SL.small(orig, est, gen, kept, mil, ops=ops, info=info2)
    if a[0] != SL.OK or info2.get("outside") or info.get("front_suffix"):
        return None
    return SL.kept_exons(a)


def three_ways(ref, host, ops, name, orig, est, gen, exons, mil):
    """one case -> (the answer, its tags, the witnesses it carries), or the end of the run"""
    q = [dict(est_off=0, est_len=len(est), first_exon=0, n_exons=len(exons), reserved=0, orig_off=0)]
    if len(orig) != len(est) or SL.einval(len(est), len(gen), exons, q):
        raise SystemExit("case %s is no query of the entry: %r" % (name, exons))
    info = {"tagged": True}
    mine = SL.small(orig, est, gen, exons, mil, ops=ops, info=info)
    tags = SL.tags_of(info)
    free_info = {"no_caps": True}
    free = SL.small(orig, est, gen, exons, mil, ops=ops, info=free_info) if mine[0] != SL.OK else mine
    outside = bool(info.get("outside") or free_info.get("outside"))
    if free[0] != SL.OK:                                     # a list out of order: the reference asserts, the host code has no rule
        return mine, tags, [2]
    witnesses = [2]
    # 1. the reference, against the composition on the same input
    want = composition(orig, est, gen, exons, mil, ops)
    if want is not None:
        got = ref.refine(orig, est, exons, mil)
        if got is not None:
            if got != want:
                raise SystemExit("case %s: refine_EST_factorizations leaves %r, the composition %r" % (name, got, want))
            witnesses.insert(0, 1)
    # 3. the host
    if not outside:
        h = host.small(orig, est, exons, mil)
        if not SL.agrees_with_host(free, h):
            raise SystemExit("case %s: ef_chain_small %r, the restatement %r" % (name, h, free))
        witnesses.append(3)
    return mine, tags + (["outside"] if outside else []), witnesses


def row(name, orig, est, exons, mil, answer, tags, witnesses):
    return [name, None if orig == est else orig.decode("latin-1"), est.decode("latin-1"), [list(e) for e in exons], mil, list(answer[:8]),
            [list(e) for e in answer[8]], list(answer[9]), tags, witnesses]


def main():
    if not RL.have_ref():
        raise SystemExit("oracle/_ref/libpintron_ref_core.so is missing: build() makes it where the reference's sources are")
    cover = {t: 0 for t in SL.TAGS}
    counts = {"hand": 0, "refused": {}, "witness": {"1": 0, "2": 0, "3": 0}, "outside": 0}
    broken = {"again": 0, "clean_on_working": 0, "external_first": 0}
    worlds = []
    for seed, gen, made in SL.make_worlds(SEED):
        ref, host, ops = Ref(gen), SL.Host(gen), SL.OracleOps(gen)
        rows = []
        try:
            for name, orig, est, exons, mil in made:
                mine, tags, wit = three_ways(ref, host, ops, name, orig, est, gen, exons, mil)
                rows.append(row(name, orig, est, exons, mil, mine, tags, wit))
                for t in tags:
                    if t in cover:
                        cover[t] += 1
                counts["hand"] += 1
                counts["outside"] += "outside" in tags
                if mine[0] != SL.OK:
                    counts["refused"][str(mine[1])] = counts["refused"].get(str(mine[1]), 0) + 1
                for k in wit:
                    counts["witness"][str(k)] += 1
                for how in broken:
                    broken[how] += SL.small(orig, est, gen, exons, mil, ops=ops, **{how: True}) != mine
        finally:
            host.close()
        original = RL.rnd(np.random.default_rng(seed), len(gen))
        if len(original) != len(gen):
            raise SystemExit("world %d: the sequence has %d bytes, its seed gives %d" % (seed, len(gen), len(original)))
        diff = np.flatnonzero(np.frombuffer(gen, np.uint8) != np.frombuffer(original, np.uint8))
        edits = []
        for p in diff.tolist():
            if edits and p == edits[-1][0] + len(edits[-1][1]):
                edits[-1][1] += chr(gen[p])
            else:
                edits.append([p, chr(gen[p])])
        worlds.append({"seed": seed, "length": len(gen), "edits": edits, "cases": rows})
    real = {}
    for source in ("c2", "ambn", "issue13"):
        genomic = TL.real_done(source)[0]
        ref, host, ops = Ref(genomic), SL.Host(genomic), SL.OracleOps(genomic)
        rows = []
        try:
            for c in TL.load_fixture()[2][source]:
                if c["answer"][:2] != (TL.OK, 0):
                    continue
                exons = TL.kept_exons(c["answer"])
                mine, tags, wit = three_ways(ref, host, ops, c["name"], c["orig"], c["est"], genomic, exons, REAL_MIL)
                rows.append(row(c["name"], c["orig"], c["est"], exons, REAL_MIL, mine, tags, wit))
                for t in tags:
                    if t in cover:
                        cover[t] += 1
                for k in wit:
                    counts["witness"][str(k)] += 1
        finally:
            host.close()
        real[source] = rows
    print(json.dumps({"cover": cover, "counts": counts, "real": {s: len(r) for s, r in real.items()}, "broken": broken}))
    short = [t for t in SL.TAGS if cover[t] < SL.MIN_PER_TAG]
    if short:
        raise SystemExit("the cover is short of: %s" % ", ".join(short))
    for how, n in broken.items():
        if n < SL.MIN_PER_TAG:
            raise SystemExit("only %d cases notice a restatement broken by `%s`" % (n, how))
    doc = {"worlds": worlds, "real": real}
    with gzip.GzipFile(SL.FIXTURE, "wb", compresslevel=9, mtime=0) as f:
        f.write(json.dumps(doc, separators=(",", ":")).encode())
    size = os.path.getsize(SL.FIXTURE)
    if size > LIMIT:
        os.remove(SL.FIXTURE)
        raise SystemExit("the fixture would take %d bytes, more than %d" % (size, LIMIT))
    n_real = sum(len(r) for r in real.values())
    with open(SL.FIXTURE[:-len(".json.gz")] + ".md", "w") as f:
        f.write("# `small_chains.json.gz`\n\nMade by `tools/make_small_golden.py`.  Data only.\n\n")
        f.write("%d hand-made factorizations over %d seeded sequences (the file lists the bytes written into each) and the "
                "factorizations of c2 (%d), test-AMBN (%d) and test-issue-13 (%d) as `tail_chains.json.gz` left them, each with "
                "its `min_intron_length` and with what the three steps of `pgpu_index_small_chains` make of it: the result "
                "fields, the list after step 2 and its step bytes.\n\n"
                % (counts["hand"], len(worlds), len(real["c2"]), len(real["ambn"]), len(real["issue13"])))
        f.write("A case is stored because its witnesses agree; a disagreement ends the tool, and no case was left out.  (1) The "
                "reference's own object code, `refine_EST_factorizations` of `libpintron_ref_core.so`, static helpers included, "
                "on its own lists, held against steps 3 to 5 of `tests/tail_lib.py` followed by the restatement of "
                "`tests/small_lib.py` on the same input.  (2) The restatement alone, whose answer is stored.  (3) The host's "
                "own routines, `ef_chain_small`.  The last field of a case lists the witnesses it carries: a case tagged "
                "`outside` (the reference would read outside a string) or `disordered`, and a case the reference's process "
                "does not survive, has no witness 1.  Cases beyond a cap are stored with their refusal and were held against "
                "the reference and the host code with the caps lifted.\n\n")
        f.write("- hand-made: %d cases; refused, by code: %s; tagged `outside`: %d\n"
                % (counts["hand"], ", ".join("%s: %d" % kv for kv in sorted(counts["refused"].items())), counts["outside"]))
        f.write("- witnesses over all %d cases: reference %d, restatement %d, host code %d\n"
                % (counts["hand"] + n_real, counts["witness"]["1"], counts["witness"]["2"], counts["witness"]["3"]))
        f.write("- cover (cases): %s\n" % ", ".join("`%s`: %d" % (t, cover[t]) for t in SL.TAGS))
        f.write("- hand-made cases that change their answer when the restatement is broken (tried once by the tool, on the CPU): "
                "an inserted exon analysed again %d, step 3 on the working sequence %d, step 3 in clean_chains' order %d\n"
                % (broken["again"], broken["clean_on_working"], broken["external_first"]))
        f.write("- prefix search: `est_start_N`, `gate_28/29` (e1len + EST_start), `cflen_5/6`, `lcf_tie_gen/est` (more than one "
                "start of the longest factor in the sequence / in the piece), `prefix_equal` / `prefix_ed` (no edit distance / "
                "one > 0), `prefix_borders_no` (refinement refused), `intron_short_by_1`, `mil_not_positive`, `not_canonical`, `lower_gtag` (a lower-case gt..ag at the exon's "
                "start, accepted), `mixed_gtag` (a mixed-case one, not canonical), "
                "`offp_below_6` / `offp_wraps` (off_p - pe), `window_256/257`, `piece_one_n` / `piece_two_n`, `at_first_bad` / "
                "`past_first_bad` (GEN_start against the first byte that is no upper-case ACGT).  Between search: "
                "`pair_gate_51/52`, `e1slen_by_gen`, `dist_2/3` (sed + ped over a classified intron), `class2_dist_0`, "
                "`extension` (the loop of :725-737 fired), `gate_f1/f2/room/elen` (that gate of :743-758 closed alone), "
                "`search_none`, `search_tie`, `winner_6`, `three_insertions`, `grow_past_64`, `exons_65`, `efact_n`.  Last "
                "cleaning: `noisy_middle_tie`, `kband_31/32`, `end_9/10/19/20` with `end_site_ok`, `end_no_donor`, "
                "`end_no_acceptor`, `end_differs`, `emptied_noisy/external`, `orig_decides` (the answer differs between the two "
                "sequences), `inserted_dropped`, `disordered`.\n")
    print("wrote %s: %d bytes (limit %d)" % (SL.FIXTURE, size, LIMIT))


if __name__ == "__main__":
    main()
