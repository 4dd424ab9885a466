"""Cost of the factorization stage (pgpu_pairing_plan_run_factorizations) on a C3-shaped chunk: the first `--ests` ESTs of
pintron_amd/synth.py's C3 (200 kb, ESTs of 600 +- 100 bases with 3 % errors), both strands, i.e. one of the ten chunks a
C3 step of 100 000 ESTs is prefetched in.

One resident plan, one process.  After warm-up rounds, `--repeats` rounds of run -> run_meg -> run_candidates, then
  (a) pgpu_pairing_plan_factorizations_ms k = 0 .. 3   HIP-event times: the whole call, clean_kernel, gaps_kernel, chain_kernel;
  (b) run_factorizations + fetch_factorizations      the two calls on the host clock: what a caller waits for;
  (c) the call-by-call route on the same candidates  pgpu_index_clean_chains, pgpu_index_gap_chains and
                                                     pgpu_index_refine_chains one after the other (tests/fact_lib.py):
                                                     their three kernel times, the seconds inside the three entries on the
                                                     host clock (uploads, validation and downloads included: the
                                                     baseline), and the whole route with its glue in Python, for the record.
Every round the plan form's bytes are compared with the route's.  Also: the outcome counts, and how many of the queries
of each stage were placeholders.  Median and range as one JSON line."""
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
    import fact_lib as F
    import pairing_lib as PL
    from pintron_amd import capi, synth
    w = synth.make("C3", n_est=a.ests)
    seqs = list(w.est_seqs) + [PL.revcomp(e) for e in w.est_seqs]
    blob = b"".join(seqs)
    off = np.zeros(len(seqs) + 1, dtype=np.uint64)
    np.cumsum([len(s) for s in seqs], out=off[1:])
    out = {"patterns": len(seqs), "bases": len(w.genomic)}
    ms = [[], [], [], []]
    wall, route_kern, route_lib, route_wall = [], [[], [], []], [], []
    with capi.Context(0) as ctx:
        idx = capi.Index(ctx, w.genomic)
        plan = capi.PairingPlan(ctx, idx, seqs, resident=True)
        for r in range(a.warmup + a.repeats):
            plan.run(15, 0.2)
            plan.run_meg()
            plan.run_candidates(15, 40)
            t0 = time.perf_counter()
            plan.run_factorizations(*F.DEFAULTS)
            res, exons, steps = plan.fetch_factorizations()
            t1 = time.perf_counter()
            cand = plan.fetch_candidates()
            q = F.plan_queries(off, cand[0])
            clock = {}
            t2 = time.perf_counter()
            r3, e3, s3 = F.call_by_call(idx, len(w.genomic), blob, cand[1], q, F.DEFAULTS, clock)
            t3 = time.perf_counter()
            r3 = F.stage0_of_kinds(r3, cand[0]["kind"])
            if r3.tobytes() != res.tobytes() or e3.tobytes() != exons.tobytes() or s3.tobytes() != steps.tobytes():
                raise SystemExit("fact_cost: the plan form and the call-by-call route disagree")
            if r >= a.warmup:
                for k in range(4):
                    ms[k].append(plan.factorizations_ms(k))
                wall.append(1e3 * (t1 - t0))
                for k in range(3):
                    route_kern[k].append(clock["kernel_ms"][k])
                route_lib.append(1e3 * clock["library_s"])
                route_wall.append(1e3 * (t3 - t2))
        o, s, d = res["outcome"], res["stage"], res["detail"]
        n = len(res)
        at_clean = int(((s == 0) | ((o == F.HOST) & (s == 1) & (d == 2))).sum())
        at_gaps = int(((s <= 1) | ((o == F.HOST) & (s == 2) & (d == 2))).sum())
        at_refine = int(((s <= 2) | ((o == F.HOST) & (s == 3) & (d == 2))).sum())
        kern = [a_ + b_ + c_ for a_, b_, c_ in zip(ms[1], ms[2], ms[3])]
        out.update(candidate_exons=int(len(cand[1])), exons=int(len(exons)),
                   outcomes={"host": int((o == F.HOST).sum()), "empty": int((o == F.EMPTY).sum()), "done": int((o == F.DONE).sum())},
                   outcome_by_stage={"%s_%d" % (("host", "empty", "done")[oo], ss): int(((o == oo) & (s == ss)).sum())
                                     for oo in range(3) for ss in range(4) if ((o == oo) & (s == ss)).any()},
                   placeholders={"clean": at_clean, "gaps": at_gaps, "refine": at_refine, "of": n},
                   factorizations_ms={"whole": spread(ms[0]), "clean": spread(ms[1]), "gaps": spread(ms[2]), "refine": spread(ms[3])},
                   not_kernels_share_of_whole=round(1.0 - statistics.median(kern) / statistics.median(ms[0]), 4),
                   run_and_fetch_factorizations_wall_ms=spread(wall),
                   route_kernels_ms={"clean": spread(route_kern[0]), "gaps": spread(route_kern[1]), "refine": spread(route_kern[2])},
                   route_inside_the_three_entries_wall_ms=spread(route_lib), route_with_python_glue_wall_ms=spread(route_wall))
        plan.close()
        idx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
