#!/usr/bin/env python3
"""Writes tests/golden/refine_introns.json.gz: what refine_intron (src/refine-intron.c:47-265) of the reference's own
object code (oracle/_ref/libpintron_ref_core.so, made by build() where the reference's sources are) returns and leaves
in the two factors, for generated introns: planted one after the other in a seeded random sequence (tests/refine_lib.py), GT-AG, GC-AG
and non-canonical sites, the borders moved by 0 - 25 bases, substitutions, indels, EST gaps, lower case and N near the
junction, first and later introns, min_intron_length on both sides of the intron's size.  Every exon lies at least 64
bases inside the sequence and inside its EST, so the reference never reads outside its strings.

The file holds data only: the edits that plant the sites, and per case the EST, the two factors, the flag, the four
settings, the return value, the two factors afterwards, and the branch (`path`) the restatement names for it.  The
rows are not stored: the tests compute them with the oracle's CPU gap alignment.  A case is kept only when the
restatement agrees with the reference on it -- a disagreement ends the run -- and the file is not written unless
every path has at least MIN_PER_PATH cases.

    python tools/make_refine_golden.py
"""
import gzip
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle_lib as O  # noqa: E402
import refine_lib as RL  # noqa: E402

MIN_PER_PATH = 25
CANDIDATES = 30000
KEEP_PER_PATH = {0: 300, 1: 300, 2: 400, 3: 400, 4: 550, 5: 500, 6: 500, 7: 250, 8: 250, 9: 400}
KEEP_REFUSED = 150            # cases of paths 5 - 9 that the test of :245 refuses, kept beside the quota


def overflows_reference(est, gen, donor, acceptor, st):
    """refine_intron allocates sequence_on_est for the donor's suffix and the acceptor's prefix alone (:84) and then
    appends the unaligned EST gap between them as well (:86-87): with a gap the string outgrows its block.  Inside the
    slack glibc leaves behind a block nothing happens; beyond it the call is undefined (and has been seen to answer
    differently), so such inputs are left out."""
    gap = acceptor[0] - donor[1] - 1
    if gap <= 0:
        return False
    se, _ = RL.gap_windows(est, gen, donor, acceptor, *st[:3])
    asked = len(se) - gap + 1
    usable = max(24, ((asked + 8 + 15) & ~15) - 8)
    return len(se) + 1 > usable


def main():
    if not RL.have_ref():
        raise SystemExit("oracle/_ref/libpintron_ref_core.so is missing: build() makes it where the reference's sources are")
    rng = np.random.default_rng(4242)
    g = bytearray(RL.fixture_genomic())
    ref = RL.RefRefiner(bytes(g))
    edits, kept, per_path, refused, skipped, crashed = [], [], [0] * RL.N_PATHS, 0, 0, 0
    pos = 200                                           # where the next kept case goes: the cases do not overlap
    for k in range(CANDIDATES):
        r = k % 10
        # aimed inputs for the rare branches: GC-AG with a moved border (the two _2 routines), sites no routine accepts
        # (Burset), exons of a few bases and exons that can change sides whole (the test of :245), a donor that belongs
        # to the acceptor (attached), a GC-AG intron beside a junction without sites (Shift_left_to_right_2)
        if r == 0:
            c = RL.make_case(rng, pos, site=(b"GC", b"AG"))
        elif r == 1:
            c = RL.make_case(rng, pos, site=None)
        elif r == 2:
            c = RL.make_case(rng, pos, site=(b"GC", b"AG"), short_exons=True)
        elif r == 3:
            c = RL.make_case(rng, pos, short_exons=True)
        elif r in (4, 6):
            c = RL.make_case(rng, pos, site=(b"GC", b"AG"), aim="gc-left")
        elif r == 5:
            c = RL.make_case(rng, pos, aim=("attached", "refused-acceptor", "refused-donor", "repeat-left", "repeat-right")[k // 10 % 5])
        else:
            c = RL.make_case(rng, pos)
        if c["ae"] + 200 > len(g):
            break
        saved = [(p, bytes(g[p:p + len(s)])) for p, s in c["edits"]]
        for p, s in c["edits"]:
            g[p:p + len(s)] = s
            ref.gen[p:p + len(s)] = s
        keep = False
        case = RL.finish_case(rng, g, c, aimed=int(rng.integers(1, 9)) if r < 4 else 0 if r < 7 else None)
        if case is not None:
            est, donor, acceptor, first, st = case
            er, gr, v = RL.oracle_rows(O, est, g, donor, acceptor, *st[:3])
            info = {}
            status, refined, path, d2, a2 = RL.refine(est, g, er, gr, v, donor, acceptor, first, *st, info=info)
            is_refused = path >= 5 and not refined
            if status != RL.OK or info["outside"] or overflows_reference(est, g, donor, acceptor, st):
                skipped += 1                            # beyond the kernel's caps, or a scan of the reference leaves its
            elif per_path[path] < KEEP_PER_PATH[path] or (is_refused and refused < KEEP_REFUSED):      # rows (undefined there)
                want = ref.refine_isolated(est, donor, acceptor, first, *st)
                if want is None:
                    crashed += 1                        # the reference's own code does not survive the call
                elif (refined, d2, a2) != want:
                    raise SystemExit("the restatement and the reference disagree on candidate %d: %r / %r\n%r" %
                                     (k, (refined, d2, a2), want, case))
                else:
                    keep = True
        if keep:
            per_path[path] += 1
            refused += is_refused
            kept.append([est.decode(), list(donor), list(acceptor), int(first), list(st), refined, list(d2), list(a2), path])
            edits += [[p, s.decode()] for p, s in c["edits"]]
            pos = c["ae"] + 21
        else:
            for p, s in reversed(saved):
                g[p:p + len(s)] = s
                ref.gen[p:p + len(s)] = s
    for p in range(RL.N_PATHS):
        print("path %d %-15s %5d cases" % (p, RL.PATH_NAMES[p], per_path[p]))
    print("skipped (undefined in the reference or beyond the caps): %d" % skipped)
    print("the reference crashed on: %d" % crashed)
    print("refused by the last test (paths 5 - 9): %d" % refused)
    short = [RL.PATH_NAMES[p] for p in range(RL.N_PATHS) if per_path[p] < MIN_PER_PATH]
    if short or refused < MIN_PER_PATH:
        raise SystemExit("not written: fewer than %d cases of %s" % (MIN_PER_PATH, ", ".join(short) or "the refused kind"))
    doc = {"source": "refine_intron of the reference's object code; path by tests/refine_lib.py",
           "genomic": "refine_lib.fixture_genomic() with `edits` [position, bytes] written into it",
           "case": "[est, donor, acceptor, first_intron, [suffpref_length_on_est, _for_intron, _on_gen, min_intron_length], "
                   "returned, donor after, acceptor after, path]; factors are [EST_start, EST_end, GEN_start, GEN_end]",
           "length": len(g), "edits": edits, "cases": kept}
    with gzip.GzipFile(RL.FIXTURE, "wb", mtime=0) as f:
        f.write(json.dumps(doc, separators=(",", ":")).encode())
    print("%d cases -> %s (%d bytes)" % (len(kept), os.path.relpath(RL.FIXTURE, ROOT), os.path.getsize(RL.FIXTURE)))


if __name__ == "__main__":
    main()
