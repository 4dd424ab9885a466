#!/usr/bin/env python3
"""Writes tests/golden/wide_chains.json.gz and wide_chains.md: the hand-made cases of tests/wide_lib.py -- lost prefix and
suffix windows and prefix windows of the small stage of 256 to 1 025 EST bytes -- with what pgpu_index_tail_chains_wide and
pgpu_index_small_chains_wide make of them.

Every case is computed three times, by the routines of tools/make_tail_golden.py and tools/make_small_golden.py with the
two caps of the restatements at their wide values, and stored only when the three agree; a disagreement ends the run, and no
case is dropped.
  1. The reference's object code (oracle/_ref/libpintron_ref_core.so and libref_harness.so, made by build() where the
     reference's sources are): find_longest_affix, compute_edit_distance and general_refine_borders as the questions of the
     tail stage, correct_composition_tail, detect_polyA_signal and remove_invalid_factorizations as they are, and
     refine_EST_factorizations for the small stage.
  2. The wide restatement, tests/wide_lib.py.
  3. The host's own routines, ef_chain_tail and ef_chain_small, which have no caps.
A case beyond a wide cap, or one that meets another cap, is stored with its refusal and held against the others with the
caps lifted.

Once, before writing, the tool runs the restatement with caps of 512 and with the genomic window of a prefix cut at 304
bytes, and checks that answers change: a fixture that such a build would pass is not written.

The file holds data only.  It is not written unless every tag of wide_lib.TAGS has wide_lib.MIN_PER_TAG cases.

    python tools/make_wide_golden.py
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
import make_small_golden as MS  # noqa: E402
import make_tail_golden as MT  # noqa: E402
import oracle_lib as O  # noqa: E402
import refine_lib as RL  # noqa: E402
import small_lib as SL  # noqa: E402
import tail_lib as TL  # noqa: E402
import wide_lib as WL  # noqa: E402

LIMIT = 1 << 20


def main():
    if not RL.have_ref() or not os.path.exists(os.path.join(O.REF_DIR, "libref_harness.so")):
        raise SystemExit("oracle/_ref/libpintron_ref_core.so or libref_harness.so is missing: build() makes them where the "
                         "reference's sources are")
    gen, tails, smalls, _ = WL.make_world()
    cover = {t: 0 for t in WL.TAGS}
    counts = {"tail": 0, "tail_refused": 0, "small": 0, "small_refused": {}, "witness": {"1": 0, "2": 0, "3": 0}}
    broken = {"cap_512": 0, "gen_304": 0}
    tail_rows, small_rows = [], []
    ref, host = MT.Ref(), TL.Host(gen)
    try:
        for name, orig, est, exons in tails:
            with WL.caps():
                mine, _, info = MT.three_ways(ref, host, name, orig, est, gen, exons)
                tags = sorted(WL.tail_tags(orig, est, gen, exons, mine, info))
                broken["gen_304"] += TL.tail(orig, est, gen, exons, ops=WL.Cut304Ops()) != mine
            with WL.caps(512, 512):
                broken["cap_512"] += TL.tail(orig, est, gen, exons) != mine
            tail_rows.append(MT.row(name, orig, est, exons, mine, tags))
            for t in tags:
                cover[t] += 1
            counts["tail"] += 1
            counts["tail_refused"] += mine[0] != TL.OK
    finally:
        host.close()
    ref, host, ops = MS.Ref(gen), SL.Host(gen), SL.OracleOps(gen)
    try:
        for name, orig, est, exons, mil in smalls:
            with WL.caps():
                mine, _, wit = MS.three_ways(ref, host, ops, name, orig, est, gen, exons, mil)
                tags = sorted(WL.small_tags(est, gen, exons, mine, {"allelen": WL.small_allelen(orig, est, gen, exons, mil, ops)}))
            with WL.caps(512, 512):
                broken["cap_512"] += SL.small(orig, est, gen, exons, mil, ops=ops) != mine
            small_rows.append(MS.row(name, orig, est, exons, mil, mine, tags, wit))
            for t in tags:
                cover[t] += 1
            counts["small"] += 1
            if mine[0] != SL.OK:
                counts["small_refused"][str(mine[1])] = counts["small_refused"].get(str(mine[1]), 0) + 1
            for k in wit:
                counts["witness"][str(k)] += 1
    finally:
        host.close()
    print(json.dumps({"cover": cover, "counts": counts, "broken": broken}))
    short = [t for t in WL.TAGS if cover[t] < WL.MIN_PER_TAG]
    if short:
        raise SystemExit("the cover is short of: %s" % ", ".join(short))
    for how, n in broken.items():
        if n < WL.MIN_PER_TAG:
            raise SystemExit("only %d cases notice a restatement broken by `%s`" % (n, how))
    original = RL.rnd(np.random.default_rng(WL.SEED), WL.GEN_LEN)
    diff = np.flatnonzero(np.frombuffer(gen, np.uint8) != np.frombuffer(original, np.uint8))
    edits = []
    for p in diff.tolist():
        if edits and p == edits[-1][0] + len(edits[-1][1]):
            edits[-1][1] += chr(gen[p])
        else:
            edits.append([p, chr(gen[p])])
    doc = {"seed": WL.SEED, "length": WL.GEN_LEN, "edits": edits, "tail": tail_rows, "small": small_rows}
    with gzip.GzipFile(WL.FIXTURE, "wb", compresslevel=9, mtime=0) as f:
        f.write(json.dumps(doc, separators=(",", ":")).encode())
    size = os.path.getsize(WL.FIXTURE)
    if size > LIMIT:
        os.remove(WL.FIXTURE)
        raise SystemExit("the fixture would take %d bytes, more than %d" % (size, LIMIT))
    with open(WL.FIXTURE[:-len(".json.gz")] + ".md", "w") as f:
        f.write("# `wide_chains.json.gz`\n\nMade by `tools/make_wide_golden.py`.  Data only.\n\n")
        f.write("%d hand-made factorizations for `pgpu_index_tail_chains_wide` and %d for `pgpu_index_small_chains_wide` over one "
                "seeded sequence of %d bases (the file lists the bytes written into it), each with the answer of the wide "
                "restatement (`tests/wide_lib.py`): the result fields, the exons or the list afterwards and the step bytes.\n\n"
                % (counts["tail"], counts["small"], WL.GEN_LEN))
        f.write("Every case was computed three times, as `tail_chains.json.gz` and `small_chains.json.gz` were, with the two caps "
                "at 1 024, and is stored because the three agree; a disagreement ends the tool, and no case was left out.  (1) "
                "The reference's object code: `find_longest_affix`, `compute_edit_distance` and `general_refine_borders` as the "
                "questions of the tail stage, and `refine_EST_factorizations` for the small stage.  (2) The wide restatement.  "
                "(3) The host's `ef_chain_tail` / `ef_chain_small`, which have no caps.  Cases beyond a cap are stored with "
                "their refusal and were held against the others with the caps lifted.\n\n")
        f.write("- tail: %d cases, %d refused by a cap; small: %d cases; refused, by code: %s\n"
                % (counts["tail"], counts["tail_refused"], counts["small"],
                   ", ".join("%s: %d" % kv for kv in sorted(counts["small_refused"].items()))))
        f.write("- witnesses of the small cases: reference %d, restatement %d, host code %d\n"
                % (counts["witness"]["1"], counts["witness"]["2"], counts["witness"]["3"]))
        f.write("- cover (cases): %s\n" % ", ".join("`%s`: %d" % (t, cover[t]) for t in WL.TAGS))
        f.write("- cases that change their answer when the restatement is broken (tried once by the tool, on the CPU): caps of "
                "512: %d; the genomic window of a lost prefix cut at 304 bytes: %d\n" % (broken["cap_512"], broken["gen_304"]))
        f.write("- `affix_N` / `window_N`: a lost window / a prefix window of N EST bytes (1025: refused); `pre_wide`, `suf_wide`, "
                "`both_wide`: a window beyond 256 bytes whose DP runs; `wide_recovered`, `wide_no_cut`, `wide_skipped` (equal "
                "first bytes: no DP at any length); `gen_1198`: the genomic window of a prefix at its largest; `gen_clipped`: "
                "cut short by GEN_start; `gs_below_es`: GEN_start < EST_start; `wide_inserted` / `wide_not_inserted`: the "
                "prefix search's outcome; `tail_wide_too`: the same list has a wide lost prefix; `tail_other_cap`, "
                "`small_other_cap`: beyond the narrow cap, inside the wide one, refused by another cap (a window of 129; a "
                "K-band of 32).\n")
    print("wrote %s: %d bytes (limit %d)" % (WL.FIXTURE, size, LIMIT))


if __name__ == "__main__":
    main()
