"""Cost and yield of the wide final stage (pgpu_pairing_plan_run_final_factorizations_wide) against the narrow one on a
C3-shaped chunk: the first `--ests` ESTs of pintron_amd/synth.py's C3 (200 kb, ESTs of 600 +- 100 bases with 3 % errors),
both strands (the chunk of tools/final_cost.py and tools/unit_cost.py).

One resident plan, one process.  After warm-up rounds, `--repeats` rounds of run -> run_meg -> run_candidates, then the
narrow and the wide form one after the other, the order swapped every round:
  run_factorizations + run_final_factorizations[_wide] + fetch_final_factorizations on the host clock (what a caller waits
  for), and pgpu_pairing_plan_final_ms k = 0 .. 2, HIP-event times: the whole second driver, the tail pair, the small pair
  (in the wide form the wide kernel lies inside its pair).
The yardstick is the narrow driver in the same process.  Every round the narrow results are compared with the first
round's, the wide ones too, and wide against narrow wherever narrow is not HOST.  Then the census: patterns HOST at the
stages 4 and 5 (by refusal code at 5), and the units run_units leaves to the host, under both; and what the remaining
refusals of the wide form are.  Median and range as one JSON line, printed and, with --out, written to that file
(profiles/wide_cost.txt is such a file; the table of DESIGN.md section 5r is copied from it by hand)."""
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


def census(res, units, FL, UL):
    o, s, d, ref = res["outcome"], res["stage"], res["detail"], res["refused"]
    host = o == FL.HOST
    v = units["verdict"]
    return {"host": int(host.sum()), "empty": int((o == FL.EMPTY).sum()), "done": int((o == FL.DONE).sum()),
            "host_by_stage": {str(k): int((host & (s == k)).sum()) for k in range(6)},
            "host_4_cap": int((host & (s == 4) & (d == 1)).sum()),
            "host_5_by_refusal": {str(k): int((host & (s == 5) & (d == 1) & (ref == k)).sum()) for k in range(1, 6)},
            "units": {"aligned": int((v == UL.U_ALIGNED).sum()), "unaligned": int((v == UL.U_UNALIGNED).sum()),
                      "host": int((v == UL.U_HOST).sum())}}


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
    import unit_lib as UL
    from pintron_amd import capi, synth
    w = synth.make("C3", n_est=a.ests)
    n = len(w.est_seqs)
    seqs = list(w.est_seqs) + [PL.revcomp(e) for e in w.est_seqs]
    uq = UL.query_array([(k, k, n + k, 0) for k in range(n)])
    out = {"patterns": len(seqs), "units": n, "bases": len(w.genomic)}
    ms = {False: [[], [], []], True: [[], [], []]}
    wall = {False: [], True: []}
    first = {}
    with capi.Context(0) as ctx:
        idx = capi.Index(ctx, w.genomic)
        plan = capi.PairingPlan(ctx, idx, seqs, resident=True)
        for r in range(a.warmup + a.repeats):
            plan.run(15, 0.2)
            plan.run_meg()
            plan.run_candidates(15, 40)
            got = {}
            for wide in ((False, True) if r % 2 == 0 else (True, False)):
                t0 = time.perf_counter()
                plan.run_factorizations(*F.DEFAULTS)
                plan.run_final_factorizations(40, wide=wide)
                got[wide] = plan.fetch_final_factorizations()
                t1 = time.perf_counter()
                if r >= a.warmup:
                    wall[wide].append(1e3 * (t1 - t0))
                    for k in range(3):
                        ms[wide][k].append(plan.final_ms(k))
                key = tuple(x.tobytes() for x in got[wide])
                if first.setdefault(wide, key) != key:
                    raise SystemExit("wide_cost: a rerun gave other bytes (wide = %r)" % wide)
            settled = got[False][0]["outcome"] != FL.HOST
            if (got[True][0]["outcome"][settled] != got[False][0]["outcome"][settled]).any() or \
                    (got[True][0]["n_exons"][settled] != got[False][0]["n_exons"][settled]).any():
                raise SystemExit("wide_cost: the wide form changed a pattern the narrow form settles")
        units = {}
        for wide in (False, True):
            plan.run_factorizations(*F.DEFAULTS)
            plan.run_final_factorizations(40, wide=wide)
            res = plan.fetch_final_factorizations()[0]
            plan.run_units(uq, 0, True)
            units[wide] = (res, plan.fetch_units()[0])
        c_n, c_w = census(*units[False], FL, UL), census(*units[True], FL, UL)
        med = lambda xs: statistics.median(xs)
        out.update(narrow={"final_ms": {"whole": spread(ms[False][0]), "tail": spread(ms[False][1]), "small": spread(ms[False][2])},
                           "run_factorizations_run_final_fetch_wall_ms": spread(wall[False]), "census": c_n},
                   wide={"final_ms": {"whole": spread(ms[True][0]), "tail": spread(ms[True][1]), "small": spread(ms[True][2])},
                         "run_factorizations_run_final_fetch_wall_ms": spread(wall[True]), "census": c_w},
                   wide_over_narrow={"whole": round(med(ms[True][0]) / med(ms[False][0]), 4), "tail": round(med(ms[True][1]) / med(ms[False][1]), 4),
                                     "small": round(med(ms[True][2]) / med(ms[False][2]), 4),
                                     "wall": round(med(wall[True]) / med(wall[False]), 4)},
                   fewer={"host_4_cap": c_n["host_4_cap"] - c_w["host_4_cap"],
                          "host_5_window": c_n["host_5_by_refusal"]["2"] - c_w["host_5_by_refusal"]["2"],
                          "host_patterns": c_n["host"] - c_w["host"], "host_units": c_n["units"]["host"] - c_w["units"]["host"]})
        plan.close()
        idx.close()
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
