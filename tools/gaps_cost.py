"""Cost of check_gap_errors chained on the resident index (pgpu_index_gap_chains) next to the same work by the device
route that existed before it, and what a C3-shaped batch looks like to the entry's caps.

One batch of 100 000 generated factorizations of one to six exons on a random 60 kb sequence (tests/gaps_lib.py:
make_world), answered (a) by the one fused call: HIP-event time of the kernel and wall time of the whole synchronous call;
(b) by today's route (tests/gaps_lib.py: device_route): every EST gap one PGPU_DP_BORDERS job with PGPU_JOB_B_GENOMIC of
ONE plan, the arithmetic around it on the host.  The host side of (b) is Python here, so its wall time is reported beside
the part of it spent inside the library's own entry points (pgpu_dp_plan_create, _launch, _sync, _fetch, _destroy; packing
the job table and decoding the results are outside that clock), with the number of jobs.  The answers are compared
first; warm-up calls, then `--repeats` timed ones of the fused call and `--route-repeats` of the route; median and range
as one JSON line.

The C3-shaped batch: the candidates of tools/clean_cost.py (the gene model of pintron_amd/synth.py's C3, ESTs of
600 +- 100 bases cut from the transcript with 3 % errors, every exon block a factor with its exact coordinates) as
pgpu_index_clean_chains leaves them: how many queries come back PGPU_ERANGE, and the lengths of their EST gaps."""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4), "n": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=100_000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--route-repeats", type=int, default=3)
    ap.add_argument("--c3", type=int, default=100_000, help="queries of the C3-shaped batch")
    a = ap.parse_args()
    import gaps_lib as GL
    from pintron_amd import capi
    gen, batch = GL.make_world(43, a.queries)
    ests, exons, q = GL.batch_arrays(batch)
    n = len(q)
    out = {"queries": n, "exons": int(len(exons)), "bases": len(gen)}
    with capi.Context(0) as ctx:
        idx = capi.Index(ctx, gen)
        rc, out_exons, out_steps, res = idx.gap_chains_raw(ests, exons, q, n)
        if rc != capi.PGPU_OK:
            raise SystemExit("gaps_cost: pgpu_index_gap_chains returned %d" % rc)
        route_wall, route_lib = [], []
        for r in range(a.route_repeats):
            clock = {}
            t0 = time.perf_counter()
            route = GL.device_route(ctx, idx, gen, batch, clock=clock)
            route_wall.append(1e3 * (time.perf_counter() - t0)); route_lib.append(1e3 * clock["library_s"])
            if r == 0:
                we, ws, wr = GL.expect_arrays(exons, route)
                if (we.tobytes(), ws.tobytes(), wr.tobytes()) != (out_exons.tobytes(), out_steps.tobytes(), res.tobytes()):
                    bad = [i for i in range(n) if res[i] != wr[i]]
                    raise SystemExit("gaps_cost: the fused call and the route disagree (first result: %r)" % (bad[:1],))
                out.update(route_jobs=clock["jobs"])
                print("gaps_cost: answers equal; route %.0f ms" % route_wall[0], file=sys.stderr, flush=True)
        kern, wall = [], []
        for r in range(a.warmup + a.repeats):
            t0 = time.perf_counter()
            rc = idx.gap_chains_raw(ests, exons, q, n)[0]
            t1 = time.perf_counter()
            if rc != capi.PGPU_OK:
                raise SystemExit("gaps_cost: pgpu_index_gap_chains returned %d" % rc)
            if r >= a.warmup:
                kern.append(idx.gap_chains_kernel_ms()); wall.append(1e3 * (t1 - t0))
        idx.close()
        out.update(refused=int((res["status"] != 0).sum()), verdicts=np.bincount(res["verdict"][res["status"] == 0], minlength=2).tolist(),
                   gaps=int(((out_steps & 0x7F) != 0).sum()),
                   fused_kernel_ms=spread(kern), fused_call_wall_ms=spread(wall),
                   route_wall_ms=spread(route_wall), route_inside_library_ms=spread(route_lib))
        if a.c3:
            import clean_cost
            import clean_lib as CL
            gen3, batch3 = clean_cost.c3_shaped(a.c3)
            e3, x3, q3 = CL.batch_arrays(batch3)
            idx3 = capi.Index(ctx, gen3)
            kept_exons, _, cr = idx3.clean_chains(e3, x3, q3)
            cleaned = []
            for i in np.flatnonzero((cr["status"] == 0) & (cr["verdict"] == 0)):
                first = int(q3[i]["first_exon"]) + int(cr[i]["first_kept"])
                est, ex = batch3[i][0], [tuple(int(v) for v in e) for e in kept_exons[first:first + int(cr[i]["n_kept"])]]
                if not GL.einval(len(est), len(gen3), ex, [dict(est_off=0, est_len=len(est), first_exon=0, n_exons=len(ex), reserved=0)]):
                    cleaned.append((est, ex))
            e4, x4, q4 = GL.batch_arrays(cleaned)
            t0 = time.perf_counter()
            rc, _, s4, r4 = idx3.gap_chains_raw(e4, x4, q4, len(q4))
            t1 = time.perf_counter()
            if rc != capi.PGPU_OK:
                raise SystemExit("gaps_cost: the C3-shaped batch returned %d" % rc)
            gap_p = np.concatenate([np.array([b[0] - a_[1] - 1 for a_, b in zip(ex, ex[1:])], dtype=np.int64) for _, ex in cleaned])
            out["c3_shaped"] = {"candidates": len(batch3), "queries": len(q4), "exons": int(len(x4)), "refused": int((r4["status"] != 0).sum()),
                                "verdicts": np.bincount(r4["verdict"][r4["status"] == 0], minlength=2).tolist(),
                                "est_gaps": {"pairs": int(len(gap_p)), "empty": int((gap_p == 0).sum()), "1-16": int(((gap_p >= 1) & (gap_p <= 16)).sum()),
                                             "17-64": int(((gap_p >= 17) & (gap_p <= 64)).sum()), "above_64": int((gap_p > 64).sum()),
                                             "max": int(gap_p.max()) if len(gap_p) else 0},
                                "kernel_ms": round(idx3.gap_chains_kernel_ms(), 4), "call_wall_ms": round(1e3 * (t1 - t0), 4)}
            idx3.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
