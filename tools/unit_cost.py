"""Cost of the unit stage (pgpu_pairing_plan_run_units) on a C3-shaped chunk: the first `--ests` ESTs of
pintron_amd/synth.py's C3 (200 kb, ESTs of 600 +- 100 bases with 3 % errors), both strands, i.e. one of the ten chunks a
C3 step of 100 000 ESTs is prefetched in (the chunk of tools/fact_cost.py and tools/final_cost.py): 2 x ests patterns,
ests units, unit k = (pattern k, pattern ests + k).

One resident plan, one process.  After warm-up rounds, `--repeats` rounds of the whole ladder up to the finals, then
run_units + fetch_units on the host clock (what a caller waits for) and pgpu_pairing_plan_units_ms, the HIP-event time of
count + scan + write.  The first round's answer is compared with the restatement (tests/unit_lib.py) on the fetched finals
and record headers, every later round's with the first.  Also the census the wiring needs -- how many units of the chunk the
device settles alone: verdicts, the strand that decided, the reasons of the UNALIGNED ones, and what the HOST units wait
for.  Median and range as one JSON line, printed and, with --out, written to that file (profiles/unit_cost.txt is such a
file; the table of DESIGN.md section 5o is copied from it by hand)."""
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
    import pairing_lib as PL
    import unit_lib as UL
    from pintron_amd import capi, synth
    w = synth.make("C3", n_est=a.ests)
    n = len(w.est_seqs)
    seqs = list(w.est_seqs) + [PL.revcomp(e) for e in w.est_seqs]
    q = UL.query_array([(k, k, n + k, 0) for k in range(n)])
    out = {"patterns": len(seqs), "units": n, "bases": len(w.genomic)}
    ms, wall, ladder = [], [], []
    first = None
    with capi.Context(0) as ctx:
        idx = capi.Index(ctx, w.genomic)
        plan = capi.PairingPlan(ctx, idx, seqs, resident=True)
        for r in range(a.warmup + a.repeats):
            t0 = time.perf_counter()
            plan.run(15, 0.2)
            plan.run_meg()
            plan.run_candidates(15, 40)
            plan.run_factorizations(*F.DEFAULTS)
            plan.run_final_factorizations(40)
            t1 = time.perf_counter()
            plan.run_units(q, 0, True)
            res, blob = plan.fetch_units()
            t2 = time.perf_counter()
            if first is None:
                fres, fex, _ = plan.fetch_final_factorizations()
                want = UL.units(fres, fex, UL.empty_bits(plan.fetch_meg()), q, 0, 1)
                if want[0].tobytes() != res.tobytes() or want[1] != blob:
                    raise SystemExit("unit_cost: the device and the restatement disagree")
                first = (res.tobytes(), blob, fres)
            elif (res.tobytes(), blob) != first[:2]:
                raise SystemExit("unit_cost: a rerun gave other bytes")
            if r >= a.warmup:
                ms.append(plan.units_ms())
                wall.append(1e3 * (t2 - t1))
                ladder.append(1e3 * (t1 - t0))
        v, s, why = res["verdict"], res["strand"], res["reason"]
        decided = first[2][res["pattern"]]
        host = v == UL.U_HOST
        out.update(blob_bytes=len(blob),
                   verdicts={"aligned": int((v == UL.U_ALIGNED).sum()), "unaligned": int((v == UL.U_UNALIGNED).sum()), "host": int(host.sum())},
                   settled_share=round(float((~host).sum()) / n, 5),
                   aligned_by_strand={"fwd": int(((v == UL.U_ALIGNED) & (s == 0)).sum()), "rev": int(((v == UL.U_ALIGNED) & (s == 1)).sum())},
                   unaligned_by_reason={name: int(((v == UL.U_UNALIGNED) & (why == k)).sum())
                                        for k, name in enumerate(("empty_outcome", "very_small_exon", "empty_graph"))},
                   forward_none_by_reason_sibling_consulted=int((s == 1).sum()),
                   host_by_strand={"fwd": int((host & (s == 0)).sum()), "rev": int((host & (s == 1)).sum())},
                   host_by_stage_detail={"%d_%d" % (st, de): int((host & (decided["stage"] == st) & (decided["detail"] == de)).sum())
                                         for st, de in sorted({(int(x), int(y)) for x, y in zip(decided["stage"][host], decided["detail"][host])})},
                   units_ms=spread(ms), run_units_and_fetch_wall_ms=spread(wall), ladder_to_the_finals_wall_ms=spread(ladder),
                   units_share_of_the_ladder=round(statistics.median(wall) / statistics.median(ladder), 5))
        plan.close()
        idx.close()
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
