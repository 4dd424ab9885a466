"""Cost of the chained cleaning steps on the resident index (pgpu_index_clean_chains) next to the same work by the device
route that existed before it, and the share of a C3-shaped batch that the entry's caps refuse.

One batch of 100 000 queries on a copy of a random 600 kb sequence: 12 500 generated candidates of one to six exons
(tests/clean_lib.py: make_case), each under eight complexity thresholds, answered (a) by the one fused call: HIP-event
time of the kernel and wall time of the whole synchronous call; (b) by today's route (tests/clean_lib.py: device_route):
a PGPU_DP_ALIGN plan for the heads, one for the tails, a PGPU_DP_KBAND `tail = 1` plan for the exon checks, with the steps'
logic on the host in between.  The host side of (b) is Python here, so its wall time is reported beside the part of it
spent inside the library's own entry points (pgpu_dp_plan_create, _launch, _sync, _fetch, _destroy: tests/clean_lib.py,
run_plan_timed; packing the job table and decoding the results are outside that clock), with the number of plans and
jobs.  The answers are compared first; warm-up calls, then `--repeats` timed ones of the fused call and `--route-repeats`
of the route; median and range as one JSON line.

The C3-shaped batch: the gene model of pintron_amd/synth.py's C3 (8 - 12 exons of 80 - 300 bp on 200 kb), ESTs of
600 +- 100 bases cut from the transcript with 3 % errors, every exon block a factor with its exact coordinates, the
default threshold of 20: how many queries come back PGPU_ERANGE."""
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

SWEEP = (20.0, 4.0, 2.0, 1.0, 0.5, 0.32, 0.3, 0.25)


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4), "n": len(xs)}


def workload(bases, distinct, seed):
    import clean_lib as CL
    import refine_lib as RL
    rng = np.random.default_rng(seed)
    g = bytearray(RL.rnd(rng, bases))
    made, pos = [], 300
    for k in range(distinct):
        est, exons, thr, end = CL.make_case(rng, g, pos, aim=CL.AIMS[k % len(CL.AIMS)], k=k)
        made.append((est, exons))
        pos = end + 20 if end + 6000 < len(g) else 300 + int(rng.integers(0, 3000))
    return bytes(g), [(est, exons, thr) for est, exons in made for thr in SWEEP]


def c3_shaped(n, seed=3):
    import clean_lib as CL
    from pintron_amd import synth
    w = synth.make("C3", n_est=1)
    gen = w.genomic
    rng = np.random.default_rng(seed)
    lens = [b - a for a, b in w.exons]
    bounds = np.cumsum([0] + lens)
    total = int(bounds[-1])
    batch = []
    for _ in range(n):
        ln = int(min(max(100, rng.normal(600, 100)), total))
        st = int(rng.integers(0, total - ln + 1))
        est, exons = bytearray(), []
        for k, (a, b) in enumerate(w.exons):
            lo, hi = max(st, int(bounds[k])), min(st + ln, int(bounds[k + 1]))
            if lo >= hi:
                continue
            g0 = a + lo - int(bounds[k])
            piece = CL.mutate(rng, gen[g0:g0 + hi - lo], 0.03) or bytearray(b"A")
            exons.append((len(est), len(est) + len(piece) - 1, g0, g0 + hi - lo - 1))
            est += piece
        batch.append((bytes(est), exons, 20.0))
    return gen, batch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=100_000)
    ap.add_argument("--bases", type=int, default=600_000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--route-repeats", type=int, default=2)
    ap.add_argument("--c3", type=int, default=100_000, help="queries of the C3-shaped batch")
    a = ap.parse_args()
    import clean_lib as CL
    from pintron_amd import capi
    gen, batch = workload(a.bases, a.queries // len(SWEEP), seed=43)
    ests, exons, q = CL.batch_arrays(batch)
    n = len(q)
    out = {"queries": n, "exons": int(len(exons)), "bases": len(gen)}
    with capi.Context(0) as ctx:
        idx = capi.Index(ctx, gen)
        rc, out_exons, out_marks, res = idx.clean_chains_raw(ests, exons, q, n)
        if rc != capi.PGPU_OK:
            raise SystemExit("clean_cost: pgpu_index_clean_chains returned %d" % rc)
        t0 = time.perf_counter()
        clock = {}
        route = CL.device_route(ctx, gen, batch, clock=clock)
        route_wall, route_lib = [1e3 * (time.perf_counter() - t0)], [1e3 * clock["library_s"]]
        we, wm, wr = CL.expect_arrays(exons, route)
        if (we.tobytes(), wm.tobytes(), wr.tobytes()) != (out_exons.tobytes(), out_marks.tobytes(), res.tobytes()):
            bad = [i for i in range(n) if res[i] != wr[i]]
            raise SystemExit("clean_cost: the fused call and the route disagree (first result: %r)" % (bad[:1],))
        out.update(route_plans=clock["plans"], route_jobs=clock["jobs"])
        print("clean_cost: answers equal; route %.0f ms" % route_wall[0], file=sys.stderr, flush=True)
        kern, wall = [], []
        for r in range(a.warmup + a.repeats):
            t0 = time.perf_counter()
            rc = idx.clean_chains_raw(ests, exons, q, n)[0]
            t1 = time.perf_counter()
            if rc != capi.PGPU_OK:
                raise SystemExit("clean_cost: pgpu_index_clean_chains returned %d" % rc)
            if r >= a.warmup:
                kern.append(idx.clean_chains_kernel_ms()); wall.append(1e3 * (t1 - t0))
        for r in range(a.route_repeats - 1):
            clock = {}
            t0 = time.perf_counter()
            CL.device_route(ctx, gen, batch, clock=clock)
            route_wall.append(1e3 * (time.perf_counter() - t0)); route_lib.append(1e3 * clock["library_s"])
        idx.close()
        out.update(refused=int((res["status"] != 0).sum()), verdicts=np.bincount(res["verdict"][res["status"] == 0], minlength=8).tolist(),
                   fused_kernel_ms=spread(kern), fused_call_wall_ms=spread(wall),
                   route_wall_ms=spread(route_wall), route_inside_library_ms=spread(route_lib))
        if a.c3:
            gen3, batch3 = c3_shaped(a.c3)
            e3, x3, q3 = CL.batch_arrays(batch3)
            idx3 = capi.Index(ctx, gen3)
            t0 = time.perf_counter()
            rc, _, _, r3 = idx3.clean_chains_raw(e3, x3, q3, len(q3))
            t1 = time.perf_counter()
            if rc != capi.PGPU_OK:
                raise SystemExit("clean_cost: the C3-shaped batch returned %d" % rc)
            out["c3_shaped"] = {"queries": len(q3), "exons": int(len(x3)), "refused": int((r3["status"] != 0).sum()),
                                "verdicts": np.bincount(r3["verdict"][r3["status"] == 0], minlength=8).tolist(),
                                "kernel_ms": round(idx3.clean_chains_kernel_ms(), 4), "call_wall_ms": round(1e3 * (t1 - t0), 4)}
            idx3.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
