#!/usr/bin/env python3
"""Writes tests/golden/candidate_lists.json.gz and candidate_lists.md: every candidate factorization of MEG records
(pgpu_pairing_plan_run_candidate_lists / pgpu_index_candidate_lists, include/pintron_gpu.h) --
  (a) the hand-made records of tests/enum_lib.py;
  (b) every record of tests/golden/candidates.json.gz that is no path and has more than two vertices, with its answer;
  (c) 200 of that file's empty graphs (a source and a sink without an edge) and 300 of its one-path cases, evenly spaced.

A case is computed by the restatement (tests/enum_lib.py) with its own Burset table, by the restatement with the
reference's frequencies where oracle/_ref/libpintron_ref_core.so is there (getBursetFrequency_adaptor on a NUL-terminated
copy of the sequence), and by ef_chain_candidates of the host code (tests/hostcheck/libestfact_check.so), and is stored
because they agree.  A disagreement ends the run.  A case the restatement calls CYCLIC or beyond a cap is not sent to the
host code, which has no cap and does not return on a cycle.  update_embedding and the enumeration are `static` in the
reference and cannot be called.  Data only.

    python tools/make_enum_golden.py
"""
import base64
import ctypes as C
import gzip
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cand_lib as CL  # noqa: E402
import enum_lib as EL  # noqa: E402
import oracle_lib as O  # noqa: E402

MAX_BYTES = 1 << 20
N_EMPTY, N_ONE_PATH = 200, 300


def spaced(items, n):
    return [items[(k * len(items)) // n] for k in range(n)]


def main():
    ref = None
    if O.have_ref():
        from make_candidates_golden import RefBurset
        ref = RefBurset()
    seqs, cand_cases = CL.load_fixture()
    todo = [("hand", "hand/" + name, rec, L, mi) for name, rec, L, mi in EL.hand_cases()]
    not_path = [c for c in cand_cases if c["kind"] == CL.NOT_PATH]
    big = [c for c in not_path if struct_nv(c["record"]) > 2]           # (some of cand_lib's hand-made records among them)
    empty = [c for c in not_path if struct_nv(c["record"]) == 2 and c["seq"] != "hand"]
    paths = [c for c in cand_cases if c["kind"] in (CL.REFUSED, CL.ONE) and c["seq"] != "hand"]
    todo += [(c["seq"], "real/" + c["name"], c["record"], c["L"], c["min_intron"]) for c in big]
    todo += [(c["seq"], "empty/" + c["name"], c["record"], c["L"], c["min_intron"]) for c in spaced(empty, N_EMPTY)]
    todo += [(c["seq"], "path/" + c["name"], c["record"], c["L"], c["min_intron"]) for c in spaced(paths, N_ONE_PATH)]
    c_copies = {name: C.create_string_buffer(g, len(g) + 2) for name, g in seqs.items()}
    cases = []
    counts = {"real": 0, "real_lists": 0, "real_cap_list": 0, "real_cap_embeddings": 0, "real_cyclic": 0, "peak": 0, "created": 0}
    for seq, name, rec, L, mi in todo:
        gen = seqs[seq]
        if CL.record_einval(rec, len(gen)):
            raise SystemExit("%s %s is no record of the entry" % (seq, name))
        info = {}
        mine = EL.candidate_lists(rec, gen, L, mi, info=info)
        if any(k in info for k in CL.NEVER):
            raise SystemExit("%s %s reaches %r" % (seq, name, info))
        if ref is not None and EL.candidate_lists(rec, gen, L, mi, burset=ref) != mine:
            raise SystemExit("%s %s: the reference's frequencies give another answer" % (seq, name))
        if mine[0] in (EL.NONE, EL.LISTS):
            host = EL.host_candidate_lists(rec, c_copies[seq], L, mi)
            if host != mine:
                raise SystemExit("%s %s: the restatement %r, the host code %r" % (seq, name, mine, host))
        if name.startswith("real/"):
            counts["real"] += 1
            counts["real_lists"] += mine[0] == EL.LISTS
            counts["real_cap_list"] += mine[:2] == (EL.RANGE, EL.CAP_LIST)
            counts["real_cap_embeddings"] += mine[:2] == (EL.RANGE, EL.CAP_EMBEDDINGS)
            counts["real_cyclic"] += mine[0] == EL.CYCLIC
            if mine[0] == EL.LISTS:
                counts["peak"] = max(counts["peak"], info["peak"])
                counts["created"] = max(counts["created"], info["created"])
        kind, detail, work, n_roots, cands = mine
        cases.append([seq, name, base64.b64encode(rec).decode(), L, mi, kind, detail, work, n_roots, cands, EL.tags_of(info)])
    cover = {t: sum(1 for c in cases if t in c[10]) for t in EL.TAGS}
    short = [t for t in EL.TAGS if cover[t] < (1 if t in EL.ONCE else 3)]
    print(json.dumps(counts), json.dumps(cover))
    if short:
        raise SystemExit("the cover is short of: %r" % short)
    kinds = [sum(1 for c in cases if c[5] == k) for k in range(4)]
    doc = {"counts": counts, "cases": cases}
    with gzip.GzipFile(EL.FIXTURE, "wb", compresslevel=9, mtime=0) as f:
        f.write(json.dumps(doc, separators=(",", ":")).encode())
    size = os.path.getsize(EL.FIXTURE)
    if size > MAX_BYTES:
        os.remove(EL.FIXTURE)
        raise SystemExit("the fixture would take %d bytes" % size)
    with open(EL.FIXTURE[:-len(".json.gz")] + ".md", "w") as f:
        f.write("# `candidate_lists.json.gz`\n\nMade by `tools/make_enum_golden.py`.  Data only.\n\n")
        f.write("%d MEG records with every candidate factorization as `pgpu_index_candidate_lists` defines them: the record, "
                "`min_factor_len`, `min_intron_length`, the kind, the detail, the work units, the roots, and per candidate its "
                "root, its embedding's length and its exons.  The records are the hand-made ones of `tests/enum_lib.py` over "
                "the seeded sequence of `tests/cand_lib.py`, every record of `candidates.json.gz` that is no path and has more "
                "than two vertices (%d), %d of its %d empty graphs (a source and a sink without an edge) and %d of its %d "
                "one-path cases, evenly spaced.  The sequences are `candidates.json.gz`'s.\n\n"
                % (len(cases), len(big), N_EMPTY, len(empty), N_ONE_PATH, len(paths)))
        f.write("`update_embedding` and the enumeration are `static` in the reference and cannot be called, so the arithmetic is "
                "pinned by the restatement (`tests/enum_lib.py`, over `cand_lib.update_embedding`), by the host code "
                "(`ef_chain_candidates`) and, indirectly, by the whole-program compares of the host code with the reference.  "
                "Every case was computed by the restatement with its own Burset table, %s, and -- unless the restatement says "
                "CYCLIC or RANGE, where the host code would not return or has no cap -- by `ef_chain_candidates`; it is stored "
                "because they agree, and a disagreement ends the tool.  `pgpu_burset.h` is checked exhaustively against the "
                "reference elsewhere.\n\n"
                % ("by the restatement with the frequencies of the reference's object code (`getBursetFrequency_adaptor`)"
                   if ref is not None else "(the reference's object code was not there when this file was made)"))
        f.write("- kinds: 0 none (flagged): %d, 1 cyclic: %d, 2 beyond a cap: %d, 3 lists: %d\n" % tuple(kinds))
        f.write("- the %d records of `candidates.json.gz` that are no path and have more than two vertices: %d answered (LISTS), "
                "%d beyond the list cap, %d beyond the embedding cap, %d cyclic (`cand_lib`'s hand-made `cycle`); among the answered the longest list ever held has %d entries and the most embeddings created "
                "for a record are %d\n" % (counts["real"], counts["real_lists"], counts["real_cap_list"],
                                           counts["real_cap_embeddings"], counts["real_cyclic"], counts["peak"], counts["created"]))
        f.write("- cover (cases): %s\n" % ", ".join("`%s`: %d" % (t, cover[t]) for t in EL.TAGS))
        f.write("- the seven outcomes of `maximality_relation` are `longer_2`, `longer_1` (add longer than the entry), "
                "`shorter_0`, `shorter_1`, `equal_0`, `equal_2`, `equal_1`; `removal_then_append`: an entry removed and add "
                "appended; `stop_at_0`: a relation 0, add dropped.  A stop at 0 with a removal in front of it cannot occur: with "
                "c1 removed by add and add stopped by c2, c1 lies inside add and add inside c2 on the pairings they share, so "
                "c1 lies inside c2, and whichever of the two came second was dropped or removed the other when it came.  "
                "`list_64` / `cap_list`: a list of exactly 64 entries, answered, and of 65, refused (three layers of four "
                "alternatives, and one way more); `embeddings_512` / `cap_embeddings`: 512 and 513 created embeddings.\n")
    print("wrote %s: %d bytes, %d cases" % (EL.FIXTURE, size, len(cases)))


def struct_nv(rec):
    import struct
    return struct.unpack_from("<I", rec, 0)[0]


if __name__ == "__main__":
    main()
