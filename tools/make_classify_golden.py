#!/usr/bin/env python3
"""Writes tests/golden/classify_introns.json.gz: (start, end, type) triples and 5' scores recorded from the
reference's own object code (oracle/_ref/libpintron_ref_core.so, made by build() where the reference's sources are),
over the AMBN genomic, one regression genomic and two seeded synthetic sequences.  Only inputs where the reference is
defined: every byte of a sequence in ACGTNacgtn, start and end inside the sequence, and the 14-byte window of the 5'
matrices (start - 3 .. start + 10) inside it too -- for a start below 3 or above len - 11 real_substring returns a
short string and GetMatInspectorScoreOfaMotif reads a matrix row that does not exist (whatever the heap holds).

    python tools/make_classify_golden.py
"""
import gzip
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import small_exon_lib as SL  # noqa: E402

SEQUENCES = [
    {"name": "ambn", "file": "tests/golden/ambn/genomic.txt"},
    {"name": "cpb2", "file": "tests/golden/regression/test-CPB2/genomic.txt.xz"},
    {"name": "synth-plain", "synth": {"seed": 101, "gen_len": 40000}},
    {"name": "synth-n-lower", "synth": {"seed": 102, "gen_len": 30000, "n_runs": [[5000, 5200], [17990, 18003]],
                                         "lower": [[9000, 12000], [29900, 30000]]}},
]
PER_SEQUENCE = 11000


PWM5_LEN = (14, 14, 13, 14)                 # GTAG-U12, ATAC-U12, GTAG-U2, GCAG-U2


def defined_start(s, n, length=14):
    return s >= 3 and s - 3 + length <= n


def pairs_of(g, rng):
    n = len(g)
    up = g.upper()
    out = set()
    # every canonical GT..AG / GC..AG / AT..AC pair inside sampled windows
    for _ in range(14):
        w0 = int(rng.integers(0, max(1, n - 700)))
        w1 = min(n, w0 + int(rng.integers(120, 700)))
        don = [i for i in range(w0, w1 - 1) if up[i:i + 2] in (b"GT", b"GC")]
        acc = [i + 1 for i in range(w0, w1 - 1) if up[i:i + 2] == b"AG"]
        adon = [i for i in range(w0, w1 - 1) if up[i:i + 2] == b"AT"]
        aacc = [i + 1 for i in range(w0, w1 - 1) if up[i:i + 2] == b"AC"]
        cand = [(s, e) for s in don for e in acc if e > s + 1] + [(s, e) for s in adon for e in aacc if e > s + 1]
        for j in rng.permutation(len(cand))[:400]:
            out.add(cand[int(j)])
    # canonical donors with far acceptors (real intron lengths)
    don = [i for i in range(n - 1) if up[i:i + 2] in (b"GT", b"GC", b"AT")]
    acc = [i + 1 for i in range(n - 1) if up[i:i + 2] in (b"AG", b"AC")]
    for _ in range(1500):
        s, e = don[int(rng.integers(len(don)))], acc[int(rng.integers(len(acc)))]
        if e > s:
            out.add((s, e))
    for _ in range(1500):                       # random pairs
        s = int(rng.integers(0, n))
        out.add((s, int(rng.integers(s, n))))
    for _ in range(60):                         # lengths 4..40 around the 30 boundary
        s = int(rng.integers(0, n - 41))
        for length in range(4, 41):
            out.add((s, s + length - 1))
    for a in acc[::max(1, len(acc) // 150)]:    # ... ending on an acceptor, starting on whatever is there
        for length in (28, 29, 30, 31, 32):
            if a - length + 1 >= 0:
                out.add((a - length + 1, a))
    for s in range(6):                          # starts 0..5 (0..2 fall to the filter below: undefined)
        for e in list(range(s, s + 45)) + [int(x) for x in rng.integers(s, n, 20)]:
            out.add((s, e))
    for s in [int(x) for x in rng.integers(0, n, 150)] + list(range(n - 60, n)):      # ends at n - 1
        out.add((s, n - 1))
    for lo in range(0, n, 997):                 # tiny introns: 1, 2, 3 bytes
        for length in (1, 2, 3):
            if lo + length <= n:
                out.add((lo, lo + length - 1))
    out = sorted((s, e) for s, e in out if defined_start(s, n))
    if len(out) > PER_SEQUENCE:
        keep = sorted(rng.permutation(len(out))[:PER_SEQUENCE].tolist())
        out = [out[i] for i in keep]
    return out


def main():
    if not SL.have_ref():
        raise SystemExit("oracle/_ref/libpintron_ref_core.so is missing: build() makes it where the reference's sources are")
    doc = {"source": "classify_genomic_intron_start_end and GetScoreOf5Prime*BySS of the reference's object code",
           "types": "0 U12, 1 U2, 2 not classified; start and end inclusive", "sequences": []}
    total = 0
    for si, entry in enumerate(SEQUENCES):
        g = SL.fixture_sequence(entry)
        assert set(g) <= set(b"ACGTNacgtn"), entry["name"]
        rng = np.random.default_rng(1000 + si)
        ref = SL.RefClassifier(g)
        n = len(g)
        triples = [[s, e, ref.classify(s, e)] for s, e in pairs_of(g, rng)]
        starts = sorted(set(list(range(0, 8)) + list(range(n - 20, n)) + [int(x) for x in rng.integers(0, n, 600)]))
        scores = [[k, s, float(ref.score5(k, s)).hex()] for s in starts for k in range(4) if defined_start(s, n, PWM5_LEN[k])]
        e = dict(entry)
        e.update(length=n, triples=[x for t in triples for x in t], score5=scores)
        doc["sequences"].append(e)
        hist = np.bincount([t[2] for t in triples], minlength=3).tolist()
        print("%-14s n=%6d  %6d triples (U12 %d, U2 %d, none %d), %d scores" % (entry["name"], n, len(triples), *hist, len(scores)))
        total += len(triples)
    with gzip.GzipFile(SL.FIXTURE, "wb", mtime=0) as f:
        f.write(json.dumps(doc, separators=(",", ":")).encode())
    print("%d triples -> %s (%d bytes)" % (total, os.path.relpath(SL.FIXTURE, ROOT), os.path.getsize(SL.FIXTURE)))


if __name__ == "__main__":
    main()
