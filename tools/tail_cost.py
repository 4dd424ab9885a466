"""Cost of the stage behind the refinement loop chained on the resident index (pgpu_index_tail_chains) next to the same
questions by the device route that exists without it, and what a C3-shaped chunk looks like to the entry.

One process.  A batch of `--queries` generated factorizations over the fixture's seeded sequence (tests/tail_lib.py:
generated), answered
  (a) by the one fused call: HIP-event time of the kernel and wall time of the whole synchronous call, after warm-up calls,
      `--repeats` times;
  (b) by the restatement over the CPU oracle, which records every question the five steps ask (longest affix, edit
      distance, border refinement); the fused call's bytes are compared with its answers first;
  (c) by ONE DP plan that holds all of those questions (PGPU_DP_AFFIX, PGPU_DP_ED, PGPU_DP_BORDERS with
      PGPU_JOB_B_GENOMIC): the seconds inside the library's own entry points (pgpu_dp_plan_create, _launch, _sync, _fetch,
      _destroy), `--route-repeats` times, the plan's answers compared with the oracle's.  This is the baseline, and it flatters
      the route: a caller does not know all questions at once (an analysis needs its edit distances before its refinement:
      tests/tail_lib.py: device_route needs one plan per round), and the glue between the questions is not in this clock.
How many queries ran a DP at all, and how many DPs of each kind, is reported for both batches.

The C3-shaped batch: the DONE factorizations of the first `--ests` ESTs of pintron_amd/synth.py's C3, both strands, as
pgpu_pairing_plan_run_factorizations leaves them (tools/fact_cost.py's chunk).  Median and range as one JSON line."""
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


class Recorder:
    """the oracle's answers, and every question with its answer"""

    def __init__(self, TL):
        self.TL, self.asked = TL, {}

    def affix(self, e, g):
        return self.asked.setdefault(("affix", e, g), self.TL.ORACLE.affix(e, g))

    def ed(self, a, b):
        return self.asked.setdefault(("ed", a, b), dict(score=self.TL.ORACLE.ed(a, b)))["score"]

    def borders(self, p, gen, gstart, gend, max_errs):
        key = ("borders", p, gstart, gend, max_errs)
        if key not in self.asked:
            self.asked[key] = self.TL.ORACLE.borders(p, gen, gstart, gend, max_errs)
        return self.asked[key]


def one_plan(ctx, idx, gen, asked, capi):
    """every recorded question in one plan -> seconds inside the library's entry points; the answers are checked"""
    keys = list(asked)
    jl = capi.JobList()
    for key in keys:
        if key[0] == "affix":
            jl.add(capi.AFFIX, key[1], key[2])
        elif key[0] == "ed":
            jl.add(capi.ED, key[1], key[2])
        else:
            _, p, gstart, gend, max_errs = key
            jl.add(capi.BORDERS, p, bytes(gend - gstart), p0=0, p1=len(p), p2=max_errs, b_gen_off=gstart, tail=min(2, len(gen) - gend))
    jobs, arena = jl.arrays()
    n = len(jl.jobs)
    res = (capi.DpResult * max(n, 1))()
    L = ctx.L
    h = C.c_void_p()
    t0 = time.perf_counter()
    rc = L.pgpu_dp_plan_create(ctx.h, idx.h, jobs, n, arena, len(arena), C.byref(h))
    rc = rc or L.pgpu_dp_plan_launch(ctx.h, h) or L.pgpu_dp_plan_sync(ctx.h, h)
    nbytes = L.pgpu_dp_plan_string_bytes(h)
    sbuf = C.create_string_buffer(max(nbytes, 1))
    rc = rc or L.pgpu_dp_plan_fetch(ctx.h, h, res, sbuf, nbytes)
    L.pgpu_dp_plan_destroy(ctx.h, h)
    inside = time.perf_counter() - t0
    ctx.check(rc)
    kinds = {"affix": capi.AFFIX, "ed": capi.ED, "borders": capi.BORDERS}
    for key, r in zip(keys, res):
        o = capi.decode(kinds[key[0]], r, b"")
        want = asked[key]
        if any(o[k] != want[k] for k in want):
            raise SystemExit("tail_cost: the plan's answer to %r is %r, the oracle's %r" % (key[0], o, want))
    return inside


def measure(ctx, idx, gen, batch, a, TL, capi, with_plan):
    ests, exons, q = TL.batch_arrays(batch)
    n = len(q)
    rc, out_exons, out_steps, res = idx.tail_chains_raw(ests, exons, q, n)
    if rc != capi.PGPU_OK:
        raise SystemExit("tail_cost: pgpu_index_tail_chains returned %d" % rc)
    rec = Recorder(TL)
    infos = [{} for _ in batch]
    want = [TL.tail(orig, est, gen, ex, ops=rec, info=i) for (_, orig, est, ex), i in zip(batch, infos)]
    we, ws, wr = TL.expect_arrays(exons, want)
    if (we.tobytes(), ws.tobytes(), wr.tobytes()) != (out_exons.tobytes(), out_steps.tobytes(), res.tobytes()):
        bad = [i for i in range(n) if res[i] != wr[i]]
        raise SystemExit("tail_cost: the fused call and the restatement disagree (first result: %r)" % (bad[:1],))
    print("tail_cost: %d answers equal the restatement's" % n, file=sys.stderr, flush=True)
    kern, wall = [], []
    for r in range(a.warmup + a.repeats):
        t0 = time.perf_counter()
        rc = idx.tail_chains_raw(ests, exons, q, n)[0]
        t1 = time.perf_counter()
        if rc != capi.PGPU_OK:
            raise SystemExit("tail_cost: pgpu_index_tail_chains returned %d" % rc)
        if r >= a.warmup:
            kern.append(idx.tail_chains_kernel_ms()); wall.append(1e3 * (t1 - t0))
    dps = {k: sum(i.get("dp_" + k, 0) for i in infos) for k in ("affix", "ed", "borders")}
    why = {}
    for i in infos:
        if "refused" in i:
            key = "".join(c for c in i["refused"] if not c.isdigit()).replace("  ", " N ")
            why[key] = why.get(key, 0) + 1
    out = {"queries": n, "exons": int(len(exons)), "est_bytes": len(ests),
           "refused": int((res["status"] != 0).sum()), "refused_for": why, "verdict_1": int(res["verdict"].sum()), "polyA": int(res["polyA"].sum()),
           "recovered": int((res["recovered"] != 0).sum()), "tail_moved": int((res["tail_added"] != 0).sum()),
           "exons_removed": int(((out_steps & 3) == 3).sum()),
           "queries_that_ran_a_dp": sum(1 for i in infos if any(i.get("dp_" + k) for k in dps)), "dps": dps,
           "distinct_questions": len(rec.asked),
           "fused_kernel_ms": spread(kern), "fused_call_wall_ms": spread(wall)}
    if with_plan and rec.asked:
        out["one_plan_inside_library_ms"] = spread([1e3 * one_plan(ctx, idx, gen, rec.asked, capi) for _ in range(a.route_repeats)])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=100_000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--route-repeats", type=int, default=3)
    ap.add_argument("--ests", type=int, default=10_000, help="ESTs of the C3-shaped chunk (0: leave it out)")
    a = ap.parse_args()
    import tail_lib as TL
    from pintron_amd import capi
    gen = TL.load_fixture()[0]
    out = {}
    with capi.Context(0) as ctx:
        idx = capi.Index(ctx, gen)
        out["generated"] = dict(measure(ctx, idx, gen, TL.generated(43, gen, a.queries), a, TL, capi, True), bases=len(gen))
        idx.close()
        if a.ests:
            import fact_lib as F
            import pairing_lib as PL
            from pintron_amd import synth
            w = synth.make("C3", n_est=a.ests)
            seqs = list(w.est_seqs) + [PL.revcomp(e) for e in w.est_seqs]
            idx = capi.Index(ctx, w.genomic)
            plan = capi.PairingPlan(ctx, idx, seqs, resident=True)
            plan.run(15, 0.2)
            plan.run_meg()
            plan.run_candidates(15, 40)
            plan.run_factorizations(*F.DEFAULTS)
            res, exons, steps = plan.fetch_factorizations()
            plan.close()
            batch = []
            for i in np.flatnonzero(res["outcome"] == F.DONE):
                lo, k = int(res[i]["first_exon"]), int(res[i]["n_exons"])
                ex = [tuple(int(v) for v in e) for e in exons[lo:lo + k]]
                est = bytes(seqs[i])
                if not TL.einval(len(est), len(w.genomic), ex, [dict(est_off=0, est_len=len(est), first_exon=0, n_exons=k, reserved=0, orig_off=0)]):
                    batch.append(("c3", est, est, ex))
            out["c3_shaped"] = dict(measure(ctx, idx, bytes(w.genomic), batch, a, TL, capi, True), patterns=len(seqs),
                                    done=int((res["outcome"] == F.DONE).sum()), bases=len(w.genomic))
            idx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
