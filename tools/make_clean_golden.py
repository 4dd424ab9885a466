#!/usr/bin/env python3
"""Writes tests/golden/clean_chains.json.gz and clean_chains.md: what the six cleaning routines of the reference's own
object code (oracle/_ref/libpintron_ref_core.so, made by build() where the reference's sources are) leave of generated
candidate factorizations -- one to six exons planted one candidate after the other in a seeded random sequence
(tests/clean_lib.py), with errors, Ns, lower case, low-complexity exons, splice sites and moved outer ends.

The file holds data only: the seed and the length of the sequence, the bytes written into it, and per candidate the EST,
the exons, the complexity threshold, the verdict, the kept run with its four outer coordinates, and -- from the restatement
alone, for the reference returns no such thing -- the mark bytes and the tags of the cover.  A candidate is stored only
when restatement and reference agree on the verdict and on the list -- a disagreement ends the run.  Candidates on which the reference's child dies, or that are beyond the entry's caps, are left
out and counted by reason; at most 1 % may be left out for a dead child.  The file is not written unless it holds the
cover the constants below ask for.

    python tools/make_clean_golden.py
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
import refine_lib as RL  # noqa: E402

SEED, GEN_LEN = 404, 1_700_000
CANDIDATES = 1150
MIN_CASES, MIN_PER_VERDICT, MIN_PER_TAG, MIN_PER_MARK = 1000, 25, 25, 25
MAX_DEAD = 0.01
COVER_TAGS = ("head_trimmed", "tail_trimmed_gap", "single", "head_dropped_of_two", "tie", "band", "odd")
VERDICT_NAMES = ("kept", "source-sink", "start/end order", "handle_endpoints", "clean_external_exons",
                 "clean_low_complexity_exons_2", "clean_noisy_exons", "check_est_coverage")


def cover(cases):
    c = {"cases": len(cases), "verdict": [0] * 8, "tags": {t: 0 for t in COVER_TAGS}, "marks": [0] * 5}
    for est, ex, thr, verdict, first, n, ends, marks, tags in cases:
        c["verdict"][verdict] += 1
        for t in COVER_TAGS:
            c["tags"][t] += t in tags
        for b in range(5):
            c["marks"][b] += any(m >> b & 1 for m in marks)
    return c


def short_of(c):
    out = []
    if c["cases"] < MIN_CASES:
        out.append("cases")
    out += ["verdict %d" % v for v in range(8) if c["verdict"][v] < MIN_PER_VERDICT]
    out += [t for t in COVER_TAGS if c["tags"][t] < MIN_PER_TAG]
    out += ["mark bit %d" % b for b in range(5) if c["marks"][b] < MIN_PER_MARK]
    return out


def main():
    if not RL.have_ref():
        raise SystemExit("oracle/_ref/libpintron_ref_core.so is missing: build() makes it where the reference's sources are")
    rng = np.random.default_rng(SEED)
    original = RL.rnd(np.random.default_rng(SEED), GEN_LEN)
    g = bytearray(original)
    made, pos = [], 200
    for k in range(CANDIDATES):
        est, exons, thr, end = CL.make_case(rng, g, pos, aim=CL.AIMS[k % len(CL.AIMS)], k=k)
        if end + 1000 > GEN_LEN:
            raise SystemExit("the sequence is too short for %d candidates" % CANDIDATES)
        made.append((est, exons, thr))
        pos = end + 20
    gen = bytes(g)
    ref = CL.RefClean(gen)
    cases, dead, beyond = [], 0, {}
    for k, (est, exons, thr) in enumerate(made):
        info = {}
        mine = CL.clean(est, gen, exons, thr, info=info)
        if mine[0] != CL.OK:
            beyond[info["refused"]] = beyond.get(info["refused"], 0) + 1
            continue
        want = ref.run(est, exons, thr)
        if want is None:
            dead += 1
            continue
        if want != CL.kept_list(mine):
            raise SystemExit("candidate %d: the reference says %r, the restatement %r\n%r" % (k, want, CL.kept_list(mine), (est, exons, thr)))
        status, verdict, first, n, ex2, marks = mine
        ends = [ex2[first][0], ex2[first][2], ex2[first + n - 1][1], ex2[first + n - 1][3]] if n else []
        cases.append((est.decode(), exons, thr, verdict, first, n, ends, marks, CL.tags_of(info)))
    c = cover(cases)
    print(json.dumps(c), "dead", dead, "beyond the caps", beyond)
    if dead > MAX_DEAD * len(made):
        raise SystemExit("%d of %d candidates left out for a dead child: more than 1 %%" % (dead, len(made)))
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
    doc = {"seed": SEED, "length": GEN_LEN, "edits": edits, "cases": cases}
    with gzip.GzipFile(CL.FIXTURE, "wb", compresslevel=9, mtime=0) as f:
        f.write(json.dumps(doc, separators=(",", ":")).encode())
    size, limit = os.path.getsize(CL.FIXTURE), os.path.getsize(RL.FIXTURE)
    if size > limit:
        os.remove(CL.FIXTURE)
        raise SystemExit("the fixture would take %d bytes, more than refine_introns.json.gz (%d)" % (size, limit))
    with open(CL.FIXTURE[:-len(".json.gz")] + ".md", "w") as f:
        f.write("# `clean_chains.json.gz`\n\nMade by `tools/make_clean_golden.py` (each candidate of the reference in a forked child).  "
                "Data only.\n\n")
        f.write("%d generated candidate factorizations with what the reference's six cleaning routines "
                "(`src/est-factorizations.c:212-244`, the routines of the reference's object code) left of them: the EST, the exons, "
                "the complexity threshold, the verdict, the kept run and its four outer coordinates.  The reference's routines "
                "return the verdict and the kept list and nothing else: those are what was compared with it.  The per-exon mark "
                "bytes stored beside them are the restatement's (`tests/clean_lib.py`); the reference bears them out only as far "
                "as the kept run implies them (an exon outside it was dropped or flagged by some step).  The candidates are "
                "planted one after the other in a seeded random sequence (the file lists the bytes written into it).\n\n" % c["cases"])
        f.write("- verdicts: %s\n" % ", ".join("%d %s: %d" % (v, VERDICT_NAMES[v], c["verdict"][v]) for v in range(8)))
        f.write("- head trimmed: %d; tail trimmed with the gap-closing loop taken: %d; single exon: %d; head dropped from a "
                "two-exon list: %d; a best-run tie: %d; a band-path end exon: %d; an `N` or lower case inside an end exon: %d\n"
                % tuple(c["tags"][t] for t in COVER_TAGS))
        f.write("- mark bits set (candidates): %s\n" % ", ".join("bit %d: %d" % (b, c["marks"][b]) for b in range(5)))
        f.write("- candidates: %d.  Left out because the reference's child died: %d.  Beyond the entry's caps: %d%s.  "
                "Restatement and reference disagreed on none (a disagreement ends the run).\n"
                % (len(made), dead, sum(beyond.values()), (" (" + "; ".join("%s: %d" % kv for kv in sorted(beyond.items())) + ")") if beyond else ""))
    print("wrote %s: %d bytes (limit %d)" % (CL.FIXTURE, size, limit))


if __name__ == "__main__":
    main()
