"""Cost of the enumeration stage (pgpu_pairing_plan_run_candidate_lists, pgpu_index_candidate_lists) on a C3-shaped chunk: the
first `--ests` ESTs of pintron_amd/synth.py's C3 (200 kb, ESTs of 600 +- 100 bases with 3 % errors), both strands, i.e. one
of the ten chunks a C3 step of 100 000 ESTs is prefetched in.

One resident plan, one process.  After warm-up rounds, `--repeats` rounds of run -> run_meg, then
  (a) pgpu_pairing_plan_meg_ms                     HIP-event time of the MEG stage's kernels, for scale;
  (b) pgpu_pairing_plan_candidate_lists_ms         HIP-event time of the stage's kernels (count + two scans + write);
  (c) run_candidate_lists + fetch_candidate_lists  the two calls on the host clock: what a caller waits for;
  (d) pgpu_index_candidate_lists                   on the same records, fetched: its kernels (HIP events) and the whole call on
                                                   the host clock, the upload of the records included;
  (e) ef_chain_candidates                          the host code over the same fetched records on one core (the records the
                                                   device refuses with a cap included: the host has none), once.
The plan form's answer is compared with the index form's, and on every record the device answers with the host code's.
What the chunk's not-path records get: answered, or which cap.  Median and range as one JSON line."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4), "n": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ests", type=int, default=10_000)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    import cand_lib as CL
    import enum_lib as EL
    import pairing_lib as PL
    from pintron_amd import capi, synth
    w = synth.make("C3", n_est=a.ests)
    seqs = list(w.est_seqs) + [PL.revcomp(e) for e in w.est_seqs]
    out = {"patterns": len(seqs), "bases": len(w.genomic)}
    meg, lists, wall, ix_kern, ix_wall = [], [], [], [], []
    with capi.Context(0) as ctx:
        idx = capi.Index(ctx, w.genomic)
        plan = capi.PairingPlan(ctx, idx, seqs, resident=True)
        for r in range(a.warmup + a.repeats):
            plan.run(15, 0.2)
            plan.run_meg()
            t0 = time.perf_counter()
            plan.run_candidate_lists(15, 40)
            res, cands, exons = plan.fetch_candidate_lists()
            t1 = time.perf_counter()
            recs = plan.fetch_meg()
            blob = b"".join(recs)
            first = np.zeros(len(recs) + 1, dtype=np.uint64)
            np.cumsum([len(x) for x in recs], out=first[1:])
            t2 = time.perf_counter()
            rc, res2, cands2, exons2, nc, ne = idx.candidate_lists_raw(blob, first, len(recs), 15, 40, len(cands), len(exons))
            t3 = time.perf_counter()
            if (rc != capi.PGPU_OK or res2.tobytes() != res.tobytes() or cands2[:nc].tobytes() != cands.tobytes()
                    or exons2[:ne].tobytes() != exons.tobytes()):
                raise SystemExit("enum_cost: the plan form and the index form disagree (rc %d)" % rc)
            if r >= a.warmup:
                meg.append(ctx.L.pgpu_pairing_plan_meg_ms(plan.h)); lists.append(plan.candidate_lists_ms()); wall.append(1e3 * (t1 - t0))
                ix_kern.append(idx.candidate_lists_kernel_ms()); ix_wall.append(1e3 * (t3 - t2))
        plan.run_candidates(15, 40)
        cres, _ = plan.fetch_candidates()
        plan.close()
        idx.close()
    # the yardstick: the host code over the same records, one core
    gen_c = C.create_string_buffer(w.genomic, len(w.genomic) + 2)
    answers = EL.answers_of_arrays(res, cands, exons)
    EL.host_candidate_lists(recs[0], gen_c, 15, 40)                         # (the library is loaded and bound outside the clock)
    t0 = time.perf_counter()
    host = [EL.host_candidate_lists(r, gen_c, 15, 40) for r in recs]
    host_ms = 1e3 * (time.perf_counter() - t0)
    differ = sum(1 for k, h in enumerate(host) if answers[k][0] in (EL.NONE, EL.LISTS) and h != answers[k])
    if differ:
        raise SystemExit("enum_cost: the device and ef_chain_candidates differ on %d records" % differ)
    not_path = cres["kind"] == CL.NOT_PATH
    kinds, detail = res["kind"][not_path], res["detail"][not_path]
    big = np.array([CL.parse(recs[k])[1].__len__() > 2 for k in np.flatnonzero(not_path)], dtype=bool)
    out.update(record_bytes=len(blob), kinds=np.bincount(res["kind"], minlength=4).tolist(), candidates=int(len(cands)),
               exons=int(len(exons)), most_candidates=int(res["n_candidates"].max()),
               not_path={"patterns": int(not_path.sum()), "more_than_two_vertices": int(big.sum()),
                         "answered": int((kinds == EL.LISTS).sum()),
                         "cap_list": int(((kinds == EL.RANGE) & (detail == EL.CAP_LIST)).sum()),
                         "cap_embeddings": int(((kinds == EL.RANGE) & (detail == EL.CAP_EMBEDDINGS)).sum()),
                         "cyclic": int((kinds == EL.CYCLIC).sum()), "flagged": int((kinds == EL.NONE).sum())},
               meg_kernels_ms=spread(meg), candidate_lists_kernels_ms=spread(lists),
               run_and_fetch_candidate_lists_wall_ms=spread(wall), index_form_kernels_ms=spread(ix_kern),
               index_form_call_wall_ms=spread(ix_wall), host_ef_chain_candidates_one_core_ms=round(host_ms, 2),
               host_ef_chain_candidates_note="through ctypes, one call per record; its per-call cost is part of the figure")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
