#!/usr/bin/env python3
"""Writes tests/golden/factorization_lists.json.gz and factorization_lists.md: the candidates of one EST to its list of
factorizations (pgpu_index_factorization_lists, include/pintron_gpu.h) --
  (a) the hand-made cases of tests/flists_lib.py (its own, the cap edges, fact_lib's one-candidate ones, and the generated
      lists that end with two or more factorizations);
  (b) every record of tests/golden/candidate_lists.json.gz's real graphs that has two or more candidates, under the
      parameter sets there, with the EST of the run it came from;
  (c) a sample of its one-candidate records and of its records without a candidate that survives.

A case is computed by the restatement (tests/flists_lib.py) and by the host code (ef_chain_factorizations on the record of a
real case, ef_chain_factorizations_from on the candidates of a hand-made one; tests/hostcheck/libestfact_check.so) and is
stored because they agree; where the restatement says HOST the host code, which has no cap, is not asked.  A disagreement
ends the run.  The merge step is held besides against the reference's own add_if_not_exists where
oracle/_ref/libpintron_ref_core.so is there: folded in a child process over the cleaned candidates, on lists built with the
reference's list_create / factor_create.  Data only.

    python tools/make_flists_golden.py
"""
import collections
import ctypes as C
import gzip
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import enum_lib as EL  # noqa: E402
import flists_lib as F  # noqa: E402
import oracle_lib as O  # noqa: E402
import refine_lib as RL  # noqa: E402

MAX_BYTES = 1 << 20
N_ONE, N_EMPTY = 60, 20


class _Node(C.Structure):
    pass


_Node._fields_ = [("next", C.POINTER(_Node)), ("prev", C.POINTER(_Node)), ("element", C.c_void_p)]


class _List(C.Structure):            # include/list.h: struct _list
    _fields_ = [("sentinel", C.POINTER(_Node)), ("size", C.c_size_t)]


def _elements(lst):
    l = C.cast(lst, C.POINTER(_List)).contents
    out, node = [], l.sentinel.contents.next
    for _ in range(l.size):
        out.append(node.contents.element)
        node = node.contents.next
    return out


class RefMerge:
    """add_if_not_exists of the reference's object code folded over lists of exons, in a child process"""

    def __init__(self):
        R = self.R = O.ref()
        R.list_create.restype = C.c_void_p
        R.list_add_to_tail.argtypes = [C.c_void_p, C.c_void_p]
        R.factor_create.restype = C.c_void_p
        R.add_if_not_exists.restype = C.c_void_p
        R.add_if_not_exists.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_bool)]

    def _fold(self, lists, max_site_difference):
        R = self.R
        cfg = RL._RefConfig()
        cfg.max_site_difference = max_site_difference
        flist = R.list_create()
        for exons in lists:
            lst = R.list_create()
            for e in exons:
                f = R.factor_create()
                C.cast(f, C.POINTER(RL._RefFactor)).contents.__init__(*e)
                R.list_add_to_tail(lst, f)
            added = C.c_bool(False)
            flist = R.add_if_not_exists(lst, flist, C.byref(cfg), C.byref(added))
        out = []
        for fl in _elements(flist):
            out.append([[x.EST_start, x.EST_end, x.GEN_start, x.GEN_end]
                        for x in (C.cast(f, C.POINTER(RL._RefFactor)).contents for f in _elements(fl))])
        return out

    def fold(self, lists, max_site_difference):
        r, w = os.pipe()
        pid = os.fork()
        if pid == 0:
            try:
                os.close(r)
                devnull = os.open(os.devnull, os.O_WRONLY)
                os.dup2(devnull, 1)
                os.dup2(devnull, 2)
                os.write(w, json.dumps(self._fold(lists, max_site_difference)).encode())
            finally:
                os._exit(0)
        os.close(w)
        data = b""
        while True:
            chunk = os.read(r, 65536)
            if not chunk:
                break
            data += chunk
        os.close(r)
        _, st = os.waitpid(pid, 0)
        if st != 0 or not data:
            return None
        return [[tuple(e) for e in x] for x in json.loads(data)]


def spaced(items, n):
    return [items[(k * len(items)) // n] for k in range(min(n, len(items)))]


def main():
    ref = RefMerge() if O.have_ref() else None
    seqs = dict(__import__("cand_lib").load_fixture()[0])
    g, hand = F.hand_cases()
    fg, fhand = F.fact_hand_as_lists()
    seqs.update({"hand": g, "fact": fg})
    todo = [("hand", "hand/" + name, est, cands, prm, None, 15) for name, est, cands, prm, _ in hand + F.cap_cases(g)]
    todo += [("hand", name, est, cands, prm, None, 15) for name, est, cands, prm, _ in F.generated_cases(g)]
    todo += [("fact", "hand/" + name, est, cands, prm, None, 15) for name, est, cands, prm, _ in fhand]
    _, ecases, _ = EL.load_fixture()
    real = [c for c in ecases if c["name"].startswith("real/") and F.real_case(c)]
    multi = [c for c in real if len(c["cands"]) >= 2]
    paths = [c for c in ecases if c["name"].startswith("path/") and F.real_case(c)]
    empty = [c for c in ecases if c["name"].startswith("empty/") and F.real_case(c)]
    for c in multi + spaced(paths, N_ONE) + spaced(empty, N_EMPTY):
        est, cands, prm = F.real_case(c)
        todo.append((c["seq"], c["name"], est, cands, prm, c["record"], c["L"]))
    hosts = {}
    ests, est_at, cases = [], {}, []
    counts = collections.Counter()
    merged_ref = 0
    for seq, name, est, cands, prm, rec, L in todo:
        gen = seqs[seq]
        info = {}
        ans = F.factorization_list(est, gen, cands, prm, info)
        if ans["outcome"] != F.HOST:
            if seq not in hosts:
                hosts[seq] = F.Host(gen)
            got = hosts[seq].factorizations(rec, est, L, prm) if rec is not None else hosts[seq].from_candidates(est, cands, prm)
            if not F.agrees_with_host(ans, got):
                raise SystemExit("%s %s: the restatement %r, the host code %r" % (seq, name, ans, got))
        if ref is not None and len(info.get("cleaned", ())) >= 2:
            theirs = ref.fold(info["cleaned"], int(prm[6]))
            if theirs != info["selected"]:
                raise SystemExit("%s %s: add_if_not_exists of the reference leaves %r, the restatement %r" % (seq, name, theirs, info["selected"]))
            merged_ref += 1
        tags = F.tags_of(ans, info)
        if est not in est_at:
            est_at[est] = len(ests)
            ests.append(est.decode())
        cases.append([name, seq, est_at[est], [[list(e) for e in x] for x in cands], list(prm), tags, F.answer_to_json(ans)])
        m2 = len(cands) >= 2
        counts["cases"] += 1
        counts["multi"] += m2
        counts["multi_host"] += m2 and ans["outcome"] == F.HOST
        counts["multi_done_2"] += m2 and ans["outcome"] == F.DONE and len(ans["facts"]) >= 2
        counts["widened"] += m2 and bool(info.get("widened"))
        if name.startswith("real/") and m2:
            counts["real_multi"] += 1
            counts["real_%s_%d" % (("host", "empty", "done")[ans["outcome"]], ans["stage"])] += 1
            counts["real_widened"] += bool(info.get("widened"))
            counts["real_two_or_more"] += ans["outcome"] == F.DONE and len(ans["facts"]) >= 2
            counts["largest_list"] = max(counts["largest_list"], info.get("listed", 0))
    for h in hosts.values():
        h.close()
    cover = {t: sum(1 for c in cases if t in c[5]) for t in F.TAGS}
    short = [t for t in F.TAGS if cover[t] < 1]
    counts["merge_held_against_reference"] = merged_ref
    print(json.dumps(counts), json.dumps(cover))
    if short:
        raise SystemExit("the cover is short of: %r" % short)
    doc = {"counts": dict(counts), "ests": ests, "cases": cases}
    with gzip.GzipFile(F.FIXTURE, "wb", compresslevel=9, mtime=0) as f:
        f.write(json.dumps(doc, separators=(",", ":")).encode())
    size = os.path.getsize(F.FIXTURE)
    if size > MAX_BYTES:
        os.remove(F.FIXTURE)
        raise SystemExit("the fixture would take %d bytes" % size)
    with open(F.FIXTURE[:-len(".json.gz")] + ".md", "w") as f:
        f.write("# `factorization_lists.json.gz`\n\nMade by `tools/make_flists_golden.py`.  Data only.\n\n")
        f.write("%d cases of `pgpu_index_factorization_lists`: an EST, its candidates in the enumeration stage's order, the nine "
                "settings, the tags, and the answer (outcome, stage, detail, the three list lengths, and per factorization its "
                "candidate, exons, step bytes, merged exons, edit total and flags).  The cases are the hand-made ones of "
                "`tests/flists_lib.py` (over its planted 30 kb sequence, and `fact_lib`'s one-candidate ones over that "
                "library's), every record of `candidate_lists.json.gz`'s real graphs with two or more candidates (%d) with the "
                "EST of its run, %d of its one-path records and %d of its empty graphs.  The sequences are `candidates.json.gz`'s.\n\n"
                % (len(cases), counts["real_multi"], min(N_ONE, len(paths)), min(N_EMPTY, len(empty))))
        f.write("Every case was computed by the restatement and, unless the restatement says HOST (the host code has no cap), by "
                "`ef_chain_factorizations` (real records) or `ef_chain_factorizations_from` (hand-made candidates); it is stored "
                "because they agree.  %s\n\n"
                % ("The merge step was held besides against the reference's own `add_if_not_exists` (object code, child process, "
                   "lists from `list_create` / `factor_create`, a `struct _configuration` with `max_site_difference` set) on the "
                   "%d cases with two or more cleaned candidates: the same lists, widened ends included." % merged_ref
                   if ref is not None else "The reference's object code was not there when this file was made, so its "
                   "`add_if_not_exists` was not called."))
        f.write("- cases with two or more candidates: %d; of them HOST: %d, DONE with two or more factorizations: %d, with a -2 "
                "widening: %d\n" % (counts["multi"], counts["multi_host"], counts["multi_done_2"], counts["widened"]))
        f.write("- the %d real records with two or more candidates: %s; DONE with two or more factorizations: %d; with a -2 "
                "widening: %d; the largest list behind `add_if_not_exists`: %d\n"
                % (counts["real_multi"], ", ".join("%s at stage %s: %d" % (k.split("_")[1].upper(), k.split("_")[2], v)
                                                    for k, v in sorted(counts.items()) if k.startswith(("real_host_", "real_empty_", "real_done_")) and k.count("_") == 2 and k.split("_")[2].isdigit()),
                   counts["real_two_or_more"], counts["real_widened"], counts["largest_list"]))
        f.write("- cover (cases per tag): %s\n" % ", ".join("`%s`: %d" % (t, cover[t]) for t in F.TAGS))
    print("wrote %s: %d bytes, %d cases" % (F.FIXTURE, size, len(cases)))


if __name__ == "__main__":
    main()
