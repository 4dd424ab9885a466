#!/usr/bin/env python3
"""Writes tests/golden/candidates.json.gz and candidates.md: the candidate factorization of MEG records
(pgpu_pairing_plan_run_candidates / pgpu_index_candidates, include/pintron_gpu.h) --
  (a) the first-attempt graphs of tests/meg_lib.py (host MEG code over the pairing oracle) of the `c2` sweep source, of
      test-AMBN and of test-issue-13, under the defaults, with both simplifications off, and with min_intron_length 0 and
      200, each as a record over the genomic sequence as the index sees it;
  (b) the hand-made records of tests/cand_lib.py for what no real graph reaches.

Every Burset frequency a case uses is the answer of the reference's object code: getBursetFrequency_adaptor of
oracle/_ref/libpintron_ref_core.so (made by build() where the reference's sources are) on a NUL-terminated copy of the
sequence.  update_embedding is `static` in the reference and cannot be called: the arithmetic around the lookup is the
restatement's (tests/cand_lib.py).  Each case is computed by the restatement with the reference's frequencies, by the
restatement with its own table, and by ef_chain_candidate of the host code (tests/hostcheck/libestfact_check.so), and is
stored because the three agree.  A disagreement ends the run.  No case is left out.

The file holds data only: per sequence its digest (the sequences are made from the inputs in the tree), and per case the
record, the two parameters, the kind, the work, the embedding's length, the exons and the tags of the cover.  It is not
written unless it holds the cover the constants below ask for.

    python tools/make_candidates_golden.py
"""
import base64
import ctypes as C
import gzip
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cand_lib as CL  # noqa: E402
import oracle_lib as O  # noqa: E402

MIN_FIVE = ("refuse_deltas", "refuse_lengths", "refuse_diagonal", "empty_range", "tie")
MAX_BYTES = 1 << 20


class RefBurset:
    """the one question, answered by the reference's object code on a NUL-terminated copy of the sequence"""

    def __init__(self):
        self.R = O.ref()
        self.R.getBursetFrequency_adaptor.restype = C.c_int
        self.R.getBursetFrequency_adaptor.argtypes = [C.c_char_p, C.c_size_t, C.c_size_t]
        self.copies = {}
        self.asked = 0

    def __call__(self, gen, cut1, cut2):
        buf = self.copies.get(id(gen))
        if buf is None:
            buf = self.copies[id(gen)] = (gen, C.create_string_buffer(gen, len(gen) + 2))     # (the adaptor reads t[cut1 + 1])
        assert 0 <= cut1 <= len(gen) and 0 <= cut2 <= len(gen)
        self.asked += 1
        return self.R.getBursetFrequency_adaptor(buf[1], cut1, cut2)


def main():
    if not O.have_ref():
        raise SystemExit("oracle/_ref/libpintron_ref_core.so is missing: build() makes it where the reference's sources are")
    ref = RefBurset()
    seqs = {"hand": CL.hand_sequence()}
    todo = [("hand", name, rec, L, mi) for name, rec, L, mi in CL.hand_cases()]
    for src, (gfa, efa) in CL.real_inputs().items():
        for set_name, prm in CL.fixture_sets():
            recs, genomic = CL.host_records(gfa, efa, prm)
            seqs.setdefault(src, genomic)
            assert seqs[src] == genomic
            todo += [(src, "%s/%d" % (set_name, k), r, prm["min_factor_len"], prm["min_intron_length"]) for k, r in enumerate(recs)]
    c_copies = {name: C.create_string_buffer(g, len(g) + 2) for name, g in seqs.items()}
    cases, scans, widest = [], 0, 0
    for seq, name, rec, L, mi in todo:
        gen = seqs[seq]
        if CL.record_einval(rec, len(gen)):
            raise SystemExit("%s %s is no record of the entry" % (seq, name))
        info = {}
        mine = CL.candidate(rec, gen, L, mi, info=info)
        want = CL.candidate(rec, gen, L, mi, burset=ref)
        host = CL.host_candidate(rec, c_copies[seq], L, mi)
        if not mine == want == host:
            raise SystemExit("%s %s: with the reference's frequencies %r, with the table %r, the host code %r" % (seq, name, want, mine, host))
        if any(k in info for k in CL.NEVER):
            raise SystemExit("%s %s reaches %r" % (seq, name, info))
        scans += info.get("scan", 0)
        widest = max(widest, info.get("widest", 0))
        kind, work, n_pairs, exons = mine
        cases.append([seq, name, base64.b64encode(rec).decode(), L, mi, kind, work, n_pairs, exons, CL.tags_of(info)])
    cov = CL.cover([dict(kind=c[5], tags=c[9]) for c in cases])
    short = [t for t in CL.TAGS if cov["tags"][t] < (5 if t in MIN_FIVE else 1)] + [k for k in range(4) if not cov["kinds"][k]]
    print(json.dumps(cov), "scans", scans, "widest", widest, "frequencies asked of the reference", ref.asked)
    if short:
        raise SystemExit("the cover is short of: %r" % short)
    hand_names = {c[1] for c in cases if c[0] == "hand"}
    if not set(CL.NOT_PATH_WAYS) <= hand_names:
        raise SystemExit("a way of not being a path is missing")
    doc = {"sequences": {n: {"length": len(g), "sha1": hashlib.sha1(g).hexdigest()} for n, g in seqs.items()}, "cases": cases}
    with gzip.GzipFile(CL.FIXTURE, "wb", compresslevel=9, mtime=0) as f:
        f.write(json.dumps(doc, separators=(",", ":")).encode())
    size = os.path.getsize(CL.FIXTURE)
    if size > MAX_BYTES:
        os.remove(CL.FIXTURE)
        raise SystemExit("the fixture would take %d bytes" % size)
    per_seq = {n: sum(1 for c in cases if c[0] == n) for n in seqs}
    with open(CL.FIXTURE[:-len(".json.gz")] + ".md", "w") as f:
        f.write("# `candidates.json.gz`\n\nMade by `tools/make_candidates_golden.py`.  Data only.\n\n")
        f.write("%d MEG records with their candidate factorization as `pgpu_index_candidates` defines it: the record, "
                "`min_factor_len`, `min_intron_length`, the kind, the work units, the embedding's length and the exons.  The "
                "records are the first-attempt graphs of `tests/meg_lib.py` (host MEG code over the pairing oracle) of the `c2` "
                "sweep source, of test-AMBN and of test-issue-13 under four parameter sets (defaults, both simplifications off, "
                "`min_intron_length` 0 and 200), and the hand-made records of `tests/cand_lib.py` over a seeded sequence of %d "
                "bases.  Every Burset frequency a case uses (%d lookups in %d cut scans, the widest of %d cuts) is the answer of "
                "the reference's object code (`getBursetFrequency_adaptor`, on a NUL-terminated copy of the sequence); "
                "`update_embedding` is `static` there, so the arithmetic around it is the restatement's.  Every case was computed "
                "three times -- the restatement with the reference's frequencies, the restatement with its own table, and "
                "`ef_chain_candidate` of the host code -- and is stored because the three agree; a disagreement ends the tool, "
                "and no case was left out.  The sequences are not in the file: the loader makes them from the inputs in the "
                "tree and checks their digests.\n\n" % (len(cases), CL.HAND_LEN, ref.asked, scans, widest))
        f.write("- cases per sequence: %s\n" % ", ".join("`%s`: %d" % kv for kv in per_seq.items()))
        f.write("- kinds: 0 none (flagged): %d, 1 not a path: %d, 2 refused: %d, 3 one candidate: %d\n" % tuple(cov["kinds"]))
        f.write("- cover (cases): %s\n" % ", ".join("`%s`: %d" % (t, cov["tags"][t]) for t in CL.TAGS))
        f.write("- `refuse_deltas` / `refuse_lengths` / `refuse_diagonal`: the three tests on `small_delta` and `big_delta`; "
                "`refuse_last`: `!(gap_on_t <= 2L || intron_on_t)`; `refuse_sink_source`: the source straight behind the sink; "
                "`split`: the overlap split, `clamp_node` / `clamp_head`: its two clamps; `scan`: a Burset cut scan ran, "
                "`empty_range`: over no cut (`best_cut` stays 0), `tie`: the best frequency more than once (the last wins); "
                "`node_at_sequence_end` / `head_at_sequence_start`: a scan whose node ends on the sequence's last byte, whose "
                "head begins on its first -- the nearest a scan comes to the adaptor's two guards (the terminator, `cut2 < 2`), "
                "which no accepted record reaches (`tests/cand_lib.py`: `NEVER`); `merged_pairing`: a pairing that moved the "
                "ends of the exon before it.\n")
    print("wrote %s: %d bytes" % (CL.FIXTURE, size))


if __name__ == "__main__":
    main()
