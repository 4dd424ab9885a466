#!/usr/bin/env python3
"""Writes tests/golden/tail_chains.json.gz and tail_chains.md: what est-fact does to a factorization directly behind the
refinement loop (correct_composition_tail, detect_polyA_signal, remove_invalid_factorizations,
recover_lost_prefixes_and_suffixes, remove_false_small_exons) on hand-made factorizations over a seeded sequence
(tests/tail_lib.py: one builder per tag of the cover) and on the DONE factorizations ef_chain_factorization gives on c2,
test-AMBN and test-issue-13.

Every case is computed three times and stored only when the three agree; a disagreement ends the run, and no case is
dropped.
  1. The reference's object code where it can be called (oracle/_ref/libpintron_ref_core.so and libref_harness.so, made by
     build() where the reference's sources are), on lists built with its own list_create / list_add_to_tail /
     factor_create: correct_composition_tail, detect_polyA_signal and remove_invalid_factorizations as they are;
     find_longest_affix (ref_static_longest_affix), compute_edit_distance and general_refine_borders as the three questions
     of steps 4 and 5.  recover_lost_prefixes_and_suffixes, remove_false_small_exons and analyze_possibly_small_exon are
     `static` in the reference and no harness exports them: the window arithmetic and the list walk around those three
     questions are the restatement's in this run.
  2. The restatement, tests/tail_lib.py, over the CPU oracle.
  3. The host's own routines, ef_chain_tail of tests/hostcheck/libestfact_check.so, over the oracle as backend.
A case in which the reference would read in front of a string (the suffix pair of an analysis with estart < esufflen or
gstart < gsufflen) is tagged `front_suffix`; none of the reference's routines called here does that read, since the
analysis around it is the restatement's.  A case beyond a cap of the entry is stored with its refusal; the host code has no
caps, so it is held against the restatement with the caps lifted.

Once, before writing, the tool leaves the re-analysis of the merged predecessor out of the restatement and checks that
the answers of the hand-made cases change: a fixture that a build without that step would pass is not written.

The file holds data only.  It is not written unless it holds the cover tests/tail_lib.py asks for.

    python tools/make_tail_golden.py
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
import ref_lib  # noqa: E402
import refine_lib as RL  # noqa: E402
import tail_lib as TL  # noqa: E402

SEED = 811
LIMIT = 1 << 20


class _Factor(C.Structure):          # include/types.h: struct _factor
    _fields_ = [("EST_start", C.c_int), ("EST_end", C.c_int), ("GEN_start", C.c_int), ("GEN_end", C.c_int)]


class _List(C.Structure):            # include/list.h: struct _list
    _fields_ = [("sentinel", C.c_void_p), ("size", C.c_size_t)]


class Ref:
    """the reference's own routines, on its own lists"""

    def __init__(self):
        R = self.R = O.ref()
        R.list_create.restype = C.c_void_p
        R.list_add_to_tail.argtypes = [C.c_void_p, C.c_void_p]
        R.factor_create.restype = C.c_void_p
        R.correct_composition_tail.restype = C.c_void_p
        R.correct_composition_tail.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p]
        R.detect_polyA_signal.restype = C.c_bool
        R.detect_polyA_signal.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.POINTER(C.c_bool)]
        R.remove_invalid_factorizations.argtypes = [C.c_void_p]

    def _list(self, exons):
        lst = self.R.list_create()
        ptrs = []
        for e in exons:
            f = self.R.factor_create()
            C.cast(f, C.POINTER(_Factor)).contents.__init__(*e)
            self.R.list_add_to_tail(lst, f)
            ptrs.append(f)
        return lst, ptrs

    def tail_and_polyA(self, orig, gen, exons):
        """-> (the last exon as correct_composition_tail left it, polyA, polyadenil)"""
        lst, ptrs = self._list(exons)
        self.R.correct_composition_tail(lst, gen, orig)
        pn = C.c_bool(False)
        pa = self.R.detect_polyA_signal(lst, gen, orig, C.byref(pn))
        t = C.cast(ptrs[-1], C.POINTER(_Factor)).contents
        return (t.EST_start, t.EST_end, t.GEN_start, t.GEN_end), int(bool(pa)), int(pn.value)

    def invalid(self, exons):
        lst, _ = self._list(exons)
        outer = self.R.list_create()
        self.R.list_add_to_tail(outer, lst)
        self.R.remove_invalid_factorizations(outer)
        return C.cast(outer, C.POINTER(_List)).contents.size == 0

    # the three questions
    def affix(self, e, g):
        return ref_lib.longest_affix(e, g)

    def ed(self, a, b):
        return ref_lib.compute_edit_distance(a, b)

    def borders(self, p, gen, gstart, gend, max_errs):
        return ref_lib.refine_borders(p, gen[gstart:gend], 0, len(p), max_errs, gen[gend:gend + 2])


def three_ways(ref, host, name, orig, est, gen, exons):
    """one case -> (the answer, its tags), or the end of the run"""
    q = [dict(est_off=0, est_len=len(est), first_exon=0, n_exons=len(exons), reserved=0, orig_off=0)]
    if len(orig) != len(est) or TL.einval(len(est), len(gen), exons, q):
        raise SystemExit("case %s is no query of the entry: %r" % (name, exons))
    info = {"tagged": True}
    mine = TL.tail(orig, est, gen, exons, info=info)
    free = TL.tail(orig, est, gen, exons, info={"no_caps": True}) if mine[0] != TL.OK else mine
    # 1. the reference
    with_ref = TL.tail(orig, est, gen, exons, ops=ref, info={"no_caps": True})
    if with_ref != free:
        raise SystemExit("case %s: with the reference's answers %r, with the oracle's %r" % (name, with_ref, free))
    tail_ex, pa, pn = ref.tail_and_polyA(orig, gen, exons)
    mine_tail = list(exons[-1])
    added = TL.correct_tail(orig, gen, mine_tail)
    if tuple(mine_tail) != tail_ex or (pa, pn) != (free[2], free[3]) or added != free[6] or (free[1] and free[7][-1] != tail_ex):
        raise SystemExit("case %s: the reference's tail and polyA %r, the restatement's %r" % (name, (tail_ex, pa, pn), (mine_tail, free[2:4])))
    if ref.invalid(list(exons[:-1]) + [tail_ex]) != bool(free[1]):
        raise SystemExit("case %s: remove_invalid_factorizations says %r" % (name, not free[1]))
    # 3. the host
    if not TL.agrees_with_host(free, host.tail(orig, est, exons)):
        raise SystemExit("case %s: ef_chain_tail %r, the restatement %r" % (name, host.tail(orig, est, exons), free))
    return mine, TL.tags_of(info), info


def row(name, orig, est, exons, answer, tags):
    return [name, None if orig == est else orig.decode(), est.decode(), [list(e) for e in exons], list(answer[:7]),
            [list(e) for e in answer[7]], list(answer[8]), tags]


def main():
    if not RL.have_ref() or not os.path.exists(os.path.join(O.REF_DIR, "libref_harness.so")):
        raise SystemExit("oracle/_ref/libpintron_ref_core.so or libref_harness.so is missing: build() makes them where the "
                         "reference's sources are")
    ref = Ref()
    original = RL.rnd(np.random.default_rng(SEED), TL.GEN_LEN)
    gen, made = TL.make_world(SEED)
    host = TL.Host(gen)
    cover = {t: 0 for t in TL.TAGS}
    counts = {"hand": 0, "refused": 0, "verdict1": 0, "dp": [0, 0, 0]}
    hand = []
    changed_without_reanalysis = 0
    try:
        for name, orig, est, exons in made:
            mine, tags, info = three_ways(ref, host, name, orig, est, gen, exons)
            hand.append(row(name, orig, est, exons, mine, tags))
            for t in tags:
                cover[t] += 1
            counts["hand"] += 1
            counts["refused"] += mine[0] != TL.OK
            counts["verdict1"] += mine[1]
            for k, key in enumerate(("dp_affix", "dp_ed", "dp_borders")):
                counts["dp"][k] += info.get(key, 0)
            changed_without_reanalysis += TL.tail(orig, est, gen, exons, reanalyse=False) != mine
    finally:
        host.close()
    real = {}
    for source in ("c2", "ambn", "issue13"):
        genomic, done = TL.real_done(source)
        host = TL.Host(genomic)
        rows = []
        try:
            for k, (est, exons) in enumerate(done):
                mine, tags, info = three_ways(ref, host, "%s-%d" % (source, k), est, est, genomic, exons)
                rows.append(row("%s-%d" % (source, k), est, est, exons, mine, tags))
                for t in tags:
                    cover[t] += 1
        finally:
            host.close()
        real[source] = rows
    print(json.dumps({"cover": cover, "counts": counts, "real": {s: len(r) for s, r in real.items()},
                      "changed_without_reanalysis": changed_without_reanalysis}))
    short = [t for t in TL.TAGS if cover[t] < TL.MIN_PER_TAG]
    if short:
        raise SystemExit("the cover is short of: %s" % ", ".join(short))
    if changed_without_reanalysis < TL.MIN_PER_TAG:
        raise SystemExit("only %d cases notice a restatement without the re-analysis after a removal" % changed_without_reanalysis)
    diff = np.flatnonzero(np.frombuffer(gen, np.uint8) != np.frombuffer(original, np.uint8))
    edits = []
    for p in diff.tolist():
        if edits and p == edits[-1][0] + len(edits[-1][1]):
            edits[-1][1] += chr(gen[p])
        else:
            edits.append([p, chr(gen[p])])
    doc = {"seed": SEED, "length": TL.GEN_LEN, "edits": edits, "cases": hand, "real": real}
    with gzip.GzipFile(TL.FIXTURE, "wb", compresslevel=9, mtime=0) as f:
        f.write(json.dumps(doc, separators=(",", ":")).encode())
    size = os.path.getsize(TL.FIXTURE)
    if size > LIMIT:
        os.remove(TL.FIXTURE)
        raise SystemExit("the fixture would take %d bytes, more than %d" % (size, LIMIT))
    with open(TL.FIXTURE[:-len(".json.gz")] + ".md", "w") as f:
        f.write("# `tail_chains.json.gz`\n\nMade by `tools/make_tail_golden.py`.  Data only.\n\n")
        f.write("%d hand-made factorizations over a seeded sequence of %d bases (the file lists the bytes written into it) and "
                "the DONE factorizations `ef_chain_factorization` gives on c2 (%d), test-AMBN (%d) and test-issue-13 (%d), each "
                "with what the five steps of `pgpu_index_tail_chains` make of it: the result fields, the exons afterwards and "
                "the step bytes.\n\n" % (counts["hand"], TL.GEN_LEN, len(real["c2"]), len(real["ambn"]), len(real["issue13"])))
        f.write("Every case was computed three times and is stored because the three agree; a disagreement ends the tool, and no "
                "case was left out.  (1) With the reference's object code where it can be called, on lists built with its own "
                "`list_create` / `list_add_to_tail` / `factor_create`: `correct_composition_tail`, `detect_polyA_signal` and "
                "`remove_invalid_factorizations` as they are, and `find_longest_affix`, `compute_edit_distance` and "
                "`general_refine_borders` as the three questions of steps 4 and 5.  `recover_lost_prefixes_and_suffixes`, "
                "`remove_false_small_exons` and `analyze_possibly_small_exon` are `static` in the reference and not exported by "
                "a harness, so the window arithmetic and the list walk around those questions are the restatement's "
                "(`tests/tail_lib.py`) in that run.  (2) With the restatement over the CPU oracle.  (3) With the host's own "
                "routines, `ef_chain_tail`.  Cases tagged `front_suffix` are the ones in which the reference would read in front "
                "of a string; no routine of the reference called here does that read.  Cases beyond a cap are stored with their "
                "refusal and were held against the host code with the caps lifted.\n\n")
        f.write("- hand-made: %d cases, %d refused by a cap, %d with verdict 1; dynamic programs run: %d affix, %d edit "
                "distance, %d border refinement\n" % (counts["hand"], counts["refused"], counts["verdict1"], *counts["dp"]))
        f.write("- cover (cases): %s\n" % ", ".join("`%s`: %d" % (t, cover[t]) for t in TL.TAGS))
        f.write("- %d hand-made cases change their answer when the re-analysis of the merged predecessor after a removal is left "
                "out of the restatement (tried once by the tool, on the CPU)\n" % changed_without_reanalysis)
        f.write("- `ext_*`: bases step 1 added; `polyA_eight`: exactly eight As behind the exon (no signal); `hex_*`: the hexamer "
                "that set polyadenil, `hex_mixed_case` / `hex_cut`: one that did not (mixed case; cut short by the sequence's "
                "end); `cancel_*`: the loop that withdrew the signal; `inv_*`: the rule that gave verdict 1; `pre_*` / `suf_*`: "
                "the lost prefix / suffix (`tie`: more than one cell of the scan has the best weight); `affix_N`: an affix "
                "window of N EST bytes whose DP ran (257: refused); `removed_twice`: the merged predecessor was removed in its "
                "re-analysis; `removed_at_1`: no prev afterwards; `burset_equal`: 2 x new == old > 0 (removed); `exon_100/101`, "
                "`window_128/129`, `gen_256/257`: the sizes at the edges of step 5's rules and caps; `orig_differs`: the two "
                "sequences of the query differ (masked ends).\n")
    print("wrote %s: %d bytes (limit %d)" % (TL.FIXTURE, size, LIMIT))


if __name__ == "__main__":
    main()
