#!/usr/bin/env python3
"""Writes tests/golden/pairing_edges.json.gz and pairing_edges.md: the pairings (MEG vertex sets) of the edge cases of
tests/pairing_edge_lib.py -- small min_factor_len, matches laid against the 16- and 32-base words, flagged bytes, byte
order, thresholds on the double's truncation, crowded lists, odd batches.

Every case goes through the CPU oracle (oracle/pairing_oracle.c) and, in a child process per genome, through the
reference's own build_vertex_set on a tree preprocessed at the case's min_factor_len (tests/pairing_lib.py: RefIndex; needs
oracle/_ref, which build() makes where the reference's sources are).  A case is stored `"by": "reference"` when the two
agree, and `"by": "oracle"` only when its genome has fewer than 64 bases (the reference's object code dies on some of
those) or the child died.  A case of 64 bases or more on which the child died or disagreed is a finding: it is listed
in the .md, stored with the oracle's answer and left out of the cover.  The file is not written unless the remaining
cases hold the cover pairing_edge_lib.cover asks for.  Data only; the same bytes at every run.

    python tools/make_pairing_edges_golden.py
"""
import gzip
import io
import json
import os
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import oracle_lib as O  # noqa: E402
import pairing_edge_lib as E  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
LIMIT = 256 * 1000


def main():
    if not O.have_ref():
        sys.exit("oracle/_ref is not built: the fixture is made where the reference's sources are")
    doc = {"seed": E.FIXTURE_SEED, "groups": {}}
    tagged, lone, fixture, findings, n_by = {}, {}, {}, [], {"reference": 0, "oracle": 0}
    for g in E.GROUPS:
        cases = E.cases(g)
        with ThreadPoolExecutor(8) as pool:                                   # one child per genome
            ref = list(pool.map(lambda c: E.reference_answers([(c[1], c[2], c[3])]), cases))
        doc["groups"][g], tagged[g], lone[g], fixture[g] = [], [], [], []
        for c, r in zip(cases, ref):
            name, gen, ests, params = c
            ans = E.oracle_answers(gen, ests, params, depths=True)
            mine = [[tri.tolist() for tri, _ in per_est] for per_est in ans]
            by, found = "reference", None
            if r is None:
                by, found = "oracle", "the reference's process died"
            elif r[0] != mine:
                by, found = "oracle", "the reference and the oracle disagree"
            if found and len(gen) >= 64:
                findings.append("`%s` (%d bases): %s" % (name, len(gen), found))
            (tagged if by == "reference" else lone)[g].append(E.tags(g, c, ans))
            n_by[by] += 1
            fixture[g].append((c, mine))
            doc["groups"][g].append({
                "name": name, "genomic": gen.decode("latin-1"), "ests": [e.decode("latin-1") for e in ests],
                "params": [list(p) for p in params], "by": by,
                "pairings": [[[v for row in tri for v in row] for tri in per_est] for per_est in mine]})
    counts, lacks = E.cover(tagged, lone)
    if lacks:
        sys.exit("the cover lacks:\n  " + "\n  ".join(lacks))
    raw = io.BytesIO()
    with gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0) as f:
        f.write(json.dumps(doc, separators=(",", ":"), sort_keys=True).encode())
    if len(raw.getvalue()) > LIMIT:
        sys.exit("pairing_edges.json.gz would hold %d bytes, above %d" % (len(raw.getvalue()), LIMIT))
    with open(os.path.join(GOLD, "pairing_edges.json.gz"), "wb") as f:
        f.write(raw.getvalue())
    seen = E.notices(fixture)
    n_cases = {g: len(doc["groups"][g]) for g in E.GROUPS}
    n_tri = {g: sum(len(flat) // 3 for c in doc["groups"][g] for per_est in c["pairings"] for flat in per_est) for g in E.GROUPS}
    with open(os.path.join(GOLD, "pairing_edges.md"), "w") as f:
        f.write("# `pairing_edges.json.gz`\n\nMade by `tools/make_pairing_edges_golden.py` from the seeded generators of "
                "`tests/pairing_edge_lib.py` (seed %d).  Data only; the tool writes the same bytes at every run.\n\n" % E.FIXTURE_SEED)
        f.write("Every case was answered by the CPU oracle (`oracle/pairing_oracle.c`) and, in a child process per genome, by the "
                "reference's own `build_vertex_set` over a tree preprocessed at the case's `min_factor_len`.  %d cases are stored "
                "`\"by\": \"reference\"`: the two agree.  %d are stored `\"by\": \"oracle\"`: " % (n_by["reference"], n_by["oracle"]))
        n_small = sum(1 for g in E.GROUPS for c in doc["groups"][g] if c["by"] == "oracle" and len(c["genomic"]) < 64)
        f.write("%d with a genome of fewer than 64 bases, on which the reference's object code died, and the %d findings below.\n\n"
                % (n_small, len(findings)))
        f.write("Findings (cases of 64 bases or more on which the reference died or disagreed; the oracle's answer is stored, "
                "and the cover does not count them): %s\n\n" % ("none." if not findings else "\n\n- " + "\n- ".join(findings)))
        f.write("The reference's process dies on every query at `min_factor_len` %s, whatever the genome, so those cases are the "
                "oracle's alone and the cover counts them apart.  It also dies on %s (the leaf hangs from the root): the generators "
                "give such a byte a second occurrence on the genome's last base.\n\n"
                % (", ".join(map(str, E.REFERENCE_DIES_AT_L)), E.UNIQUE_FIRST_BYTE))
        f.write("| group | cases | pairings |\n|---|---|---|\n")
        for g in E.GROUPS:
            f.write("| `%s` | %d | %d |\n" % (g, n_cases[g], n_tri[g]))
        f.write("\nCover, counted by the tag functions of `tests/pairing_edge_lib.py` over the cases above "
                "(`tests/test_pairing_edges_cpu.py` asks for it again):\n\n| what | count |\n|---|---|\n")
        for k, v in counts.items():
            f.write("| %s | %s |\n" % (k, v))
        f.write("\nWhat the fixture notices (the oracle alone, on changed inputs):\n\n| what | count |\n|---|---|\n")
        for k, v in seen.items():
            f.write("| %s | %s |\n" % (k, v))
    print("pairing_edges.json.gz: %d bytes, %d cases (%d by the reference), %d findings"
          % (len(raw.getvalue()), sum(n_cases.values()), n_by["reference"], len(findings)))
    for k, v in list(counts.items()) + list(seen.items()):
        print("  %-90s %s" % (k, v))


if __name__ == "__main__":
    sys.exit(main())
