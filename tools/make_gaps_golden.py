#!/usr/bin/env python3
"""Writes tests/golden/gap_chains.json.gz and gap_chains.md: check_gap_errors (src/est-factorizations.c:1462-1545) on
generated factorizations -- one to six exons planted in a seeded random sequence of 60 kb (tests/gaps_lib.py), with EST
gaps cut from the ends of their introns or made of random bases, Ns and lower case.

The border answers are the reference's object code: general_refine_borders of oracle/_ref/libpintron_ref_core.so (made by
build() where the reference's sources are) through tests/ref_lib.py, with t as its own NUL-terminated copy, as
real_substring hands it over.  check_gap_errors itself is `static` in the reference and cannot be called: the dozen lines
of arithmetic around the call (the four ends moved, the sum against the threshold, the merging loop) are the
restatement's, tests/gaps_lib.py, in both runs.  A case is stored only when the oracle-backed restatement and the
reference-backed run agree; a disagreement ends the run.  No case is left out: general_refine_borders is defined on every
input the entry accepts.

The file holds data only: the seed and the length of the sequence, the bytes written into it, and per case the EST, the
exons, the verdict, the total, the number of exons kept, the exons afterwards, the step bytes and the tags of the cover.
It is not written unless it holds the cover the constants below ask for.

    python tools/make_gaps_golden.py
"""
import gzip
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import clean_lib as CL  # noqa: E402
import gaps_lib as GL  # noqa: E402
import ref_lib  # noqa: E402
import refine_lib as RL  # noqa: E402

SEED, CASES = 1462, 1120
MIN_CASES, MIN_PER_VERDICT, MIN_PER_TAG = 1000, 100, 25


class RefOps:
    """the one question, answered by the reference's object code"""

    def borders(self, p, t, gen_off):
        return ref_lib.refine_borders(p, t, 0, len(p), len(p))


def cover(cases):
    c = {"cases": len(cases), "verdict": [0, 0], "tags": {t: 0 for t in GL.TAGS}, "gaps": 0}
    for est, ex, verdict, total, kept, after, steps, tags in cases:
        c["verdict"][verdict] += 1
        c["gaps"] += sum(1 for s in steps if s & 0x7F)
        for t in GL.TAGS:
            c["tags"][t] += t in tags
    return c


def short_of(c):
    out = ["cases"] if c["cases"] < MIN_CASES else []
    out += ["verdict %d" % v for v in range(2) if c["verdict"][v] < MIN_PER_VERDICT]
    out += [t for t in GL.TAGS if c["tags"][t] < MIN_PER_TAG]
    return out


def main():
    if not RL.have_ref():
        raise SystemExit("oracle/_ref/libpintron_ref_core.so is missing: build() makes it where the reference's sources are")
    original = RL.rnd(np.random.default_rng(SEED), GL.GEN_LEN)
    gen, made = GL.make_world(SEED, CASES)
    ref = RefOps()
    cases = []
    for k, (est, exons) in enumerate(made):
        q = [dict(est_off=0, est_len=len(est), first_exon=0, n_exons=len(exons), reserved=0)]
        if GL.einval(len(est), len(gen), exons, q):
            raise SystemExit("case %d is no query of the entry: %r" % (k, (est, exons)))
        info = {}
        mine = GL.gaps(est, gen, exons, info=info)
        want = GL.gaps(est, gen, exons, ops=ref)
        if mine != want:
            raise SystemExit("case %d: with the reference's answers %r, with the oracle's %r\n%r" % (k, want, mine, (est, exons)))
        if mine[0] != GL.OK:
            raise SystemExit("case %d is beyond the entry's caps: %r" % (k, info))
        status, verdict, total, kept, after, steps = mine
        cases.append((est.decode(), exons, verdict, total, kept, after, steps, GL.tags_of(info)))
    c = cover(cases)
    print(json.dumps(c))
    if short_of(c):
        raise SystemExit("the cover is short of: %s" % ", ".join(short_of(c)))
    # the bytes planted into the sequence, as runs that differ from the seeded one
    diff = np.flatnonzero(np.frombuffer(gen, np.uint8) != np.frombuffer(original, np.uint8))
    edits = []
    for p in diff.tolist():
        if edits and p == edits[-1][0] + len(edits[-1][1]):
            edits[-1][1] += chr(gen[p])
        else:
            edits.append([p, chr(gen[p])])
    doc = {"seed": SEED, "length": GL.GEN_LEN, "edits": edits, "cases": cases}
    with gzip.GzipFile(GL.FIXTURE, "wb", compresslevel=9, mtime=0) as f:
        f.write(json.dumps(doc, separators=(",", ":")).encode())
    size, limit = os.path.getsize(GL.FIXTURE), os.path.getsize(CL.FIXTURE)
    if size > limit:
        os.remove(GL.FIXTURE)
        raise SystemExit("the fixture would take %d bytes, more than clean_chains.json.gz (%d)" % (size, limit))
    with open(GL.FIXTURE[:-len(".json.gz")] + ".md", "w") as f:
        f.write("# `gap_chains.json.gz`\n\nMade by `tools/make_gaps_golden.py`.  Data only.\n\n")
        f.write("%d generated factorizations with what `check_gap_errors` (`src/est-factorizations.c:1462-1545`) makes of them: "
                "the EST, the exons, the verdict, the summed edit distance, the number of exons kept, the exons afterwards and "
                "the step bytes of `pgpu_index_gap_chains`.  The border refinement of each of the %d EST gaps is the answer of "
                "the reference's object code (`general_refine_borders`, with `t` as its own NUL-terminated copy); "
                "`check_gap_errors` itself is `static` there, so the arithmetic around that call is the restatement's "
                "(`tests/gaps_lib.py`).  Every case was computed twice, with the reference's refinements and with the CPU "
                "oracle's, and is stored because the two runs agree; a disagreement ends the tool, and no case was left out.  "
                "The factorizations are planted in a seeded random sequence of %d bases (the file lists the bytes written "
                "into it).\n\n" % (c["cases"], c["gaps"], GL.GEN_LEN))
        f.write("- verdicts: 0 kept: %d, 1 dropped (more than 20 errors): %d\n" % tuple(c["verdict"]))
        f.write("- cover (cases): %s\n" % ", ".join("`%s`: %d" % (t, c["tags"][t]) for t in GL.TAGS))
        f.write("- `merged_run`: two consecutive exons merged into one donor; `short_window`: gapT < 2 gapP; `gap_equals_intron`: "
                "gapT == gapP; `burset_tie`: the cut differs when the Burset frequency is ignored; `total_20` / `total_21`: the "
                "sum on either side of the threshold; `gap_64`: an EST gap at the cap; `no_gap`: every EST gap empty; "
                "`lower_or_N`: an N or lower case inside a gap or its window.\n")
    print("wrote %s: %d bytes (limit %d)" % (GL.FIXTURE, size, limit))


if __name__ == "__main__":
    main()
