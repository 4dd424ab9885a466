"""Cost of the final stage (pgpu_pairing_plan_run_final_factorizations) on a C3-shaped chunk: the first `--ests` ESTs of
pintron_amd/synth.py's C3 (200 kb, ESTs of 600 +- 100 bases with 3 % errors), both strands, i.e. one of the ten chunks a
C3 step of 100 000 ESTs is prefetched in (the chunk of tools/fact_cost.py).

One resident plan, one process.  After warm-up rounds, `--repeats` rounds of run -> run_meg -> run_candidates, then
  (a) the fused call   run_factorizations + run_final_factorizations + fetch_final_factorizations on the host clock: what a
                       caller waits for; and pgpu_pairing_plan_final_ms k = 0 .. 2, HIP-event times: the whole second
                       driver, tail_kernel, small_kernel;
  (b) today's route    run_factorizations + fetch_factorizations + pgpu_index_tail_chains + pgpu_index_small_chains on the
                       same chunk, the glue in numpy and Python (tests/final_lib.py: glue): the seconds inside the entries
                       on the host clock (uploads, validation and downloads included: the baseline), the two kernel times,
                       and the whole route with its glue, for the record.
Every round the bytes of both are compared first.  Also: the outcome counts and the share of HOST per stage.  Median and
range as one JSON line, printed and, with --out, written to that file (profiles/final_cost.txt is such a file; the table
of DESIGN.md section 5n is copied from it by hand)."""
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
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    import fact_lib as F
    import final_lib as FL
    import pairing_lib as PL
    from pintron_amd import capi, synth
    w = synth.make("C3", n_est=a.ests)
    seqs = list(w.est_seqs) + [PL.revcomp(e) for e in w.est_seqs]
    blob = b"".join(seqs)
    off = np.zeros(len(seqs) + 1, dtype=np.uint64)
    np.cumsum([len(s) for s in seqs], out=off[1:])
    out = {"patterns": len(seqs), "bases": len(w.genomic)}
    ms = [[], [], []]
    fused_wall, fact_wall, route_kern, route_lib, route_wall = [], [], [[], []], [], []
    with capi.Context(0) as ctx:
        idx = capi.Index(ctx, w.genomic)
        plan = capi.PairingPlan(ctx, idx, seqs, resident=True)
        for r in range(a.warmup + a.repeats):
            plan.run(15, 0.2)
            plan.run_meg()
            plan.run_candidates(15, 40)
            cand = plan.fetch_candidates()
            q = FL.plan_queries(off, cand[0])
            # (a) the fused call
            t0 = time.perf_counter()
            plan.run_factorizations(*F.DEFAULTS)
            plan.run_final_factorizations(40)
            res, exons, steps = plan.fetch_final_factorizations()
            t1 = time.perf_counter()
            # (b) today's route: the factorizations fetched, then the two chained entries with the glue on the host
            clock = {}
            t2 = time.perf_counter()
            plan.run_factorizations(*F.DEFAULTS)
            fact = plan.fetch_factorizations()
            t3 = time.perf_counter()
            r3, e3, s3 = FL.glue(idx, len(w.genomic), blob, q, fact, 40, clock)
            t4 = time.perf_counter()
            if r3.tobytes() != res.tobytes() or e3.tobytes() != exons.tobytes() or s3.tobytes() != steps.tobytes():
                raise SystemExit("final_cost: the plan form and today's route disagree")
            if r >= a.warmup:
                for k in range(3):
                    ms[k].append(plan.final_ms(k))
                fused_wall.append(1e3 * (t1 - t0))
                fact_wall.append(1e3 * (t3 - t2))
                for k in range(2):
                    route_kern[k].append(clock["kernel_ms"][k])
                route_lib.append(1e3 * (t3 - t2 + clock["library_s"]))
                route_wall.append(1e3 * (t4 - t2))
        o, s = res["outcome"], res["stage"]
        n = len(res)
        out.update(candidate_exons=int(len(cand[1])), exons=int(len(exons)),
                   outcomes={"host": int((o == FL.HOST).sum()), "empty": int((o == FL.EMPTY).sum()), "done": int((o == FL.DONE).sum())},
                   outcome_by_stage={"%s_%d" % (("host", "empty", "done")[oo], ss): int(((o == oo) & (s == ss)).sum())
                                     for oo in range(3) for ss in range(6) if ((o == oo) & (s == ss)).any()},
                   host_share_by_stage={str(ss): round(float(((o == FL.HOST) & (s == ss)).sum()) / n, 5) for ss in range(6)},
                   final_ms={"whole": spread(ms[0]), "tail": spread(ms[1]), "small": spread(ms[2])},
                   fused_run_factorizations_run_final_fetch_wall_ms=spread(fused_wall),
                   route_run_and_fetch_factorizations_wall_ms=spread(fact_wall),
                   route_kernels_ms={"tail": spread(route_kern[0]), "small": spread(route_kern[1])},
                   route_inside_the_entries_wall_ms=spread(route_lib), route_with_python_glue_wall_ms=spread(route_wall),
                   fused_over_route_inside_the_entries=round(statistics.median(fused_wall) / statistics.median(route_lib), 4))
        plan.close()
        idx.close()
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
