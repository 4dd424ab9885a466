#!/usr/bin/env python3
"""Writes tests/golden/refine_chains.json.gz and refine_chains.md: what the reference's refinement loop
(src/est-factorizations.c:446-490) over refine_intron of the reference's own object code
(oracle/_ref/libpintron_ref_core.so, made by build() where the reference's sources are) leaves of generated
factorizations: two to seven exons, the introns planted one after the other in a seeded random sequence
(tests/chain_lib.py over tests/refine_lib.py), sites of every kind, moved borders, noise at the junctions.

The file holds data only: the edits that plant the sites, and per chain the EST, the exons, the four settings, the
number of introns done, the first-exon flag, the exons afterwards and the step bytes (path | refined << 7) the
restatement names.  A chain is kept only when restatement and reference agree on every exon, on every return value
and on the first-exon rule -- a disagreement ends the run.  Chains on which the reference is undefined (its
sequence_on_est overflows, a scan leaves its rows) or does not survive are left out and counted.  The file is not
written unless it holds the cover the constants below ask for.

    python tools/make_chain_golden.py
"""
import gzip
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import chain_lib as CL  # noqa: E402
import refine_lib as RL  # noqa: E402
from make_refine_golden import overflows_reference  # noqa: E402

CANDIDATES = 9000
MIN_CHAINS, MIN_PER_LENGTH, MIN_PER_PATH, MIN_DROPPED, MIN_REAL_CHAINS, MIN_GAP, MIN_ODD = 1000, 150, 25, 25, 100, 25, 25
KEEP_PER_LENGTH = {2: 220, 3: 220, 4: 220, 5: 220}       # 5 stands for five exons and more
KEEP_FOR_COVER = 40                                       # beside the quota: chains that add to a count still short


def length_class(n):
    return min(n, 5)


def cover(chains):
    """the counts the fixture must reach, from (est, exons, settings, done, dropped, exons_after, steps, real, gap, odd)"""
    c = {"chains": len(chains), "length": {k: 0 for k in (2, 3, 4, 5)}, "first": [0] * RL.N_PATHS, "later": [0] * RL.N_PATHS,
         "dropped": 0, "real": 0, "gap": 0, "odd": 0}
    for ch in chains:
        c["length"][length_class(len(ch[1]))] += 1
        for i, s in enumerate(ch[6][1:]):
            c["first" if i == 0 else "later"][s & 15] += 1
        c["dropped"] += ch[4]
        c["real"] += ch[7]
        c["gap"] += ch[8]
        c["odd"] += ch[9]
    return c


def short_of(c):
    out = []
    if c["chains"] < MIN_CHAINS:
        out.append("chains")
    out += ["%d exons" % k for k in (2, 3, 4, 5) if c["length"][k] < MIN_PER_LENGTH]
    out += ["path %d at a first intron" % p for p in CL.PATHS_FIRST if c["first"][p] < MIN_PER_PATH]
    out += ["path %d at a later intron" % p for p in CL.PATHS_LATER if c["later"][p] < MIN_PER_PATH]
    for key, least in (("dropped", MIN_DROPPED), ("real", MIN_REAL_CHAINS), ("gap", MIN_GAP), ("odd", MIN_ODD)):
        if c[key] < least:
            out.append(key)
    return out


def main():
    if not RL.have_ref():
        raise SystemExit("oracle/_ref/libpintron_ref_core.so is missing: build() makes it where the reference's sources are")
    rng = np.random.default_rng(5151)
    g = bytearray(RL.fixture_genomic())
    ref = CL.RefChain(bytes(g))
    edits, kept = [], []
    undefined = crashed = beyond = not_wanted = made = 0
    pos = 200
    aims_cycle = ("attached", "gc-left", "refused-acceptor", "gc-left", "refused-donor", "repeat-left", "gc-left", "repeat-right")
    for k in range(CANDIDATES):
        n_exons = (2, 3, 4, 5, 3, 4, 5, 6, 2, 7)[k % 10]
        aims = None
        if k % 3 == 0:                                   # an aimed intron at the first place, or at a later one
            aims = [None] * (n_exons - 1)
            if k % 2 == 0:                               # Shift_left_to_right_2 is the rarest branch: every other one aims at it
                aims[0] = "gc-left" if k // 6 % 2 == 0 else aims_cycle[k // 12 % len(aims_cycle)]
            else:
                aims[int(rng.integers(n_exons - 1))] = aims_cycle[k // 3 % len(aims_cycle)]
        before = bytes(g[pos:pos + 8000])
        made_chain = CL.make_chain(rng, g, pos, n_exons, aims)
        if made_chain is None:
            if pos + 9000 > len(g):
                break
            continue
        made += 1
        est, exons, st, ch_edits, end = made_chain
        keep = False
        info = {}
        status, done, dropped, ex2, steps = CL.chain(est, bytes(g), exons, st, info=info)
        if status != CL.OK:
            beyond += 1
        elif info["outside"] or any(overflows_reference(est, g, d, a, st) for _, _, d, a in info["windows"]):
            undefined += 1
        else:
            real = int(CL.is_a_chain(est, bytes(g), exons, st, (ex2, steps)))
            row = (est, exons, st, done, dropped, ex2, steps, real, int(CL.has_est_gap(exons)),
                   int(CL.odd_bases_near_a_junction(est, exons)))
            now = cover(kept)
            lc = length_class(n_exons)
            then = cover(kept + [row])
            adds = len(short_of(then)) < len(short_of(now)) or \
                any(then[key] > now[key] and now[key] < least + KEEP_FOR_COVER
                    for key, least in (("dropped", MIN_DROPPED), ("real", MIN_REAL_CHAINS), ("gap", MIN_GAP), ("odd", MIN_ODD)))
            rare = any((now["first" if i == 0 else "later"][s & 15]) < MIN_PER_PATH + KEEP_FOR_COVER for i, s in enumerate(steps[1:]))
            if now["length"][lc] < KEEP_PER_LENGTH[lc] or adds or rare:
                for p, s in ch_edits:                    # the reference reads its own copy of the sequence
                    ref.gen[p:p + len(s)] = s
                want = ref.run(est, exons, st)
                if want is None:
                    crashed += 1
                elif want != (dropped, ex2, [s >> 7 for s in steps]):
                    raise SystemExit("the restatement and the reference disagree on candidate %d: %r / %r\n%r" %
                                     (k, (dropped, ex2, [s >> 7 for s in steps]), want, (est, exons, st)))
                else:
                    keep = True
            else:
                not_wanted += 1
        if keep:
            kept.append(row)
            edits += [[p, s.decode()] for p, s in ch_edits]
            pos = end + 21
        else:
            g[pos:pos + 8000] = before
            ref.gen[pos:pos + 8000] = before
    c = cover(kept)
    for key in ("chains", "length", "first", "later", "dropped", "real", "gap", "odd"):
        print("%-8s %s" % (key, c[key]))
    left_out = undefined + crashed
    print("candidates: %d; left out because the reference is undefined there or crashed: %d (%d + %d); beyond the caps: %d; "
          "agreed but not needed: %d" % (made, left_out, undefined, crashed, beyond, not_wanted))
    short = short_of(c)
    if short:
        raise SystemExit("not written: short of " + ", ".join(short))
    doc = {"source": "the loop of est-factorizations.c:446-490 over refine_intron of the reference's object code; steps by "
                     "tests/chain_lib.py",
           "genomic": "refine_lib.fixture_genomic() with `edits` [position, bytes] written into it",
           "chain": "[est, exons, [suffpref_length_on_est, _for_intron, _on_gen, min_intron_length], introns done, first exon "
                    "dropped, exons afterwards, steps (path | refined << 7, one per exon)]; an exon is [EST_start, EST_end, "
                    "GEN_start, GEN_end]",
           "length": len(g), "edits": edits,
           "chains": [[r[0].decode(), [list(e) for e in r[1]], list(r[2]), r[3], r[4], [list(e) for e in r[5]], list(r[6])] for r in kept]}
    with gzip.GzipFile(CL.FIXTURE, "wb", mtime=0) as f:
        f.write(json.dumps(doc, separators=(",", ":")).encode())
    size = os.path.getsize(CL.FIXTURE)
    limit = os.path.getsize(RL.FIXTURE)
    if size > limit:
        os.remove(CL.FIXTURE)
        raise SystemExit("not written: %d bytes, more than refine_introns.json.gz (%d)" % (size, limit))
    names = RL.PATH_NAMES
    with open(CL.FIXTURE.replace(".json.gz", ".md"), "w") as f:
        f.write("# `refine_chains.json.gz`\n\nMade by `tools/make_chain_golden.py` (each chain of the reference in a forked child).  "
                "Data only.\n\n")
        f.write("%d generated factorizations with what the reference's refinement loop (`src/est-factorizations.c:446-490`, "
                "`refine_intron` of the reference's object code) left of them: the EST, the exons, the three window lengths and "
                "`min_intron_length`, the exons afterwards, whether the first exon is dropped (`:476-485`), and per exon the step "
                "byte (`path | refined << 7`) `tests/chain_lib.py` names for the intron in front of it.  The introns are planted one "
                "after the other in a seeded random sequence (the file lists the bytes written into it).\n\n" % c["chains"])
        f.write("- exons per chain: %s\n" % ", ".join("%s: %d" % ("5 and more" if k == 5 else k, c["length"][k]) for k in (2, 3, 4, 5)))
        f.write("- paths at a chain's first intron: %s\n" % ", ".join("%s %d" % (names[p], c["first"][p]) for p in CL.PATHS_FIRST))
        f.write("- paths at a later intron: %s\n" % ", ".join("%s %d" % (names[p], c["later"][p]) for p in CL.PATHS_LATER))
        f.write("- `attached-first` needs `first_intron`, which the loop sets for a chain's first intron alone, and `attached-later` "
                "needs it unset: each can occur at one kind of place only.\n")
        f.write("- first exon dropped: %d; answer differs from refining every intron alone from the original exons: %d; an "
                "unaligned EST gap: %d; lower case or `N` near a junction: %d\n" % (c["dropped"], c["real"], c["gap"], c["odd"]))
        f.write("- candidates: %d.  Left out because the reference is not defined there (its `sequence_on_est` outgrows its "
                "block, `:84-87`, or a scan leaves the rows) or did not survive the call: %d (%d undefined, %d crashed).  Beyond the "
                "entry's caps: %d.  Not needed for the cover, and so neither run through the reference nor stored: %d.\n" % (made, left_out, undefined, crashed, beyond, not_wanted))
    print("%d chains -> %s (%d bytes)" % (len(kept), os.path.relpath(CL.FIXTURE, ROOT), size))


if __name__ == "__main__":
    main()
