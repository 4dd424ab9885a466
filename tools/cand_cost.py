"""Cost of the candidate stage (pgpu_pairing_plan_run_candidates, pgpu_index_candidates) on a C3-shaped chunk: the first
`--ests` ESTs of pintron_amd/synth.py's C3 (200 kb, ESTs of 600 +- 100 bases with 3 % errors), both strands, i.e. one of
the ten chunks a C3 step of 100 000 ESTs is prefetched in.

One resident plan, one process.  After warm-up rounds, `--repeats` rounds of run -> run_meg, then alternating
  (a) pgpu_pairing_plan_meg_ms           HIP-event time of the MEG stage's kernels (build + scan + emit), for scale;
  (b) pgpu_pairing_plan_candidates_ms    HIP-event time of the candidate stage's kernels (count + scan + write);
  (c) run_candidates + fetch_candidates  the two calls on the host clock: what a caller waits for;
  (d) pgpu_index_candidates              on the same records, fetched: its kernels (HIP events) and the whole call on
                                         the host clock, the upload of the records included.
The plan form's answer is compared with the index form's first.  Median and range as one JSON line."""
import argparse
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
    import pairing_lib as PL
    from pintron_amd import capi, synth
    w = synth.make("C3", n_est=a.ests)
    seqs = list(w.est_seqs) + [PL.revcomp(e) for e in w.est_seqs]
    out = {"patterns": len(seqs), "bases": len(w.genomic)}
    meg, cand, wall, ix_kern, ix_wall = [], [], [], [], []
    with capi.Context(0) as ctx:
        idx = capi.Index(ctx, w.genomic)
        plan = capi.PairingPlan(ctx, idx, seqs, resident=True)
        for r in range(a.warmup + a.repeats):
            plan.run(15, 0.2)
            plan.run_meg()
            t0 = time.perf_counter()
            plan.run_candidates(15, 40)
            res, exons = plan.fetch_candidates()
            t1 = time.perf_counter()
            recs = plan.fetch_meg()
            blob = b"".join(recs)
            first = np.zeros(len(recs) + 1, dtype=np.uint64)
            np.cumsum([len(x) for x in recs], out=first[1:])
            t2 = time.perf_counter()
            rc, res2, exons2, total = idx.candidates_raw(blob, first, len(recs), 15, 40, len(exons))
            t3 = time.perf_counter()
            if rc != capi.PGPU_OK or res2.tobytes() != res.tobytes() or exons2[:total].tobytes() != exons.tobytes():
                raise SystemExit("cand_cost: the plan form and the index form disagree (rc %d)" % rc)
            if r >= a.warmup:
                meg.append(ctx.L.pgpu_pairing_plan_meg_ms(plan.h)); cand.append(plan.candidates_ms()); wall.append(1e3 * (t1 - t0))
                ix_kern.append(idx.candidates_kernel_ms()); ix_wall.append(1e3 * (t3 - t2))
        out.update(record_bytes=len(blob), kinds=np.bincount(res["kind"], minlength=4).tolist(), exons=int(len(exons)),
                   pairings_in_candidates=int(res["n_pairs"].sum()),
                   meg_kernels_ms=spread(meg), candidates_kernels_ms=spread(cand), run_and_fetch_candidates_wall_ms=spread(wall),
                   index_form_kernels_ms=spread(ix_kern), index_form_call_wall_ms=spread(ix_wall))
        plan.close()
        idx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
