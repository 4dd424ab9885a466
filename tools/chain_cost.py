"""Cost of the chained refinement on the resident index (pgpu_index_refine_chains) next to the same work by the device
route that existed before it.

One batch of 100 000 chains on a random 200 kb sequence: 12 500 generated factorizations of two to six exons
(tests/chain_lib.py), each under eight settings (two window triples, four min_intron_length), answered (a) by the one
fused call: HIP-event time of the kernel and wall time of the whole synchronous call; (b) in rounds, one per intron
depth: the windows of that depth cut on the host from the exons as they stand, one PGPU_DP_GAP plan, one
pgpu_index_refine_introns call (tests/chain_lib.py: device_rounds).  The host side of (b) is Python here, so its wall
time is reported beside the part of it spent inside the two library calls.  The answers are compared first; warm-up
calls, then `--repeats` timed ones, the two routes alternating; median and range as one JSON line.  The fused call
allocates its per-wave workspace (16 waves per compute unit, about 98 KB each) and frees it inside the call: a
hipMalloc + hipFree of that size is timed on its own, in the same process, to show its share of the call."""
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


def workspace_alloc_ms(cus, repeats):
    """hipMalloc + hipFree of about the workspace of a full grid, by host clock; None where the runtime cannot be reached"""
    import ctypes as C
    try:
        hip = C.CDLL("libamdhip64.so")
        hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        hip.hipFree.argtypes = [C.c_void_p]
        import chain_lib as CL
        # about what the call allocates: per wave the direction bytes at the caps plus 2 KB for the strings, the windows
        # and the result (the library rounds its own sum to 100 096 B and takes the CU count from the device)
        size = cus * 16 * ((CL.MAX_GEN_WINDOW + 64) * 64 * 4 + 2048)
        out = []
        for _ in range(repeats + 1):
            p = C.c_void_p()
            t0 = time.perf_counter()
            if hip.hipMalloc(C.byref(p), size) != 0:
                return None
            hip.hipFree(p)
            out.append(1e3 * (time.perf_counter() - t0))
        return {"bytes": size, **spread(out[1:])}
    except (OSError, AttributeError):
        return None


def workload(bases, distinct, seed):
    import chain_lib as CL
    import refine_lib as RL
    rng = np.random.default_rng(seed)
    g = bytearray(RL.rnd(rng, bases))
    made, pos = [], 300
    while len(made) < distinct:
        c = CL.make_chain(rng, g, pos, int(rng.integers(2, 7)))
        if c is None:
            pos = 300 + int(rng.integers(0, 5000)) if pos + 9000 > len(g) else pos + 1
            continue
        made.append(c[:3])
        pos = c[4] + 21 if c[4] + 9000 < len(g) else 300 + int(rng.integers(0, 5000))
    gen = bytes(g)
    batch = []
    for est, exons, st in made:
        ilen = exons[1][2] - exons[0][3] - 1
        for sp in (st[:3], (30, 70, 30) if st[:3] != (30, 70, 30) else (25, 60, 35)):
            for mil in (4, 40, ilen, ilen + 25):
                batch.append((est, exons, sp + (mil,)))
    return gen, batch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=100_000)
    ap.add_argument("--bases", type=int, default=200_000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--cus", type=int, default=256, help="compute units of the device (sizes the workspace that is timed)")
    a = ap.parse_args()
    import chain_lib as CL
    from pintron_amd import capi
    gen, batch = workload(a.bases, a.chains // 8, seed=41)
    ests, exons, q = CL.batch_arrays(batch)
    n = len(q)
    with capi.Context(0) as ctx:
        idx = capi.Index(ctx, gen)
        rc, out_exons, out_steps, res = idx.refine_chains_raw(ests, exons, q, n)
        if rc != capi.PGPU_OK:
            raise SystemExit("chain_cost: pgpu_index_refine_chains returned %d" % rc)
        keep = [i for i in range(n) if res[i]["status"] == capi.PGPU_OK]        # the rounds serve what fits the caps
        if len(keep) != n:
            batch = [batch[i] for i in keep]
            ests, exons, q = CL.batch_arrays(batch)
            n = len(q)
            rc, out_exons, out_steps, res = idx.refine_chains_raw(ests, exons, q, n)
        rounds = CL.device_rounds(ctx, idx, gen, batch)
        k = 0
        for i, (ex2, steps) in enumerate(rounds):
            m = len(ex2)
            if [tuple(int(v) for v in e) for e in out_exons[k:k + m]] != ex2 or out_steps[k:k + m].tolist() != steps:
                raise SystemExit("chain_cost: the fused call and the rounds disagree on chain %d" % i)
            k += m
        kern, wall, rounds_wall, rounds_lib = [], [], [], []
        for r in range(a.warmup + a.repeats):                 # the two routes alternate: they see the same machine
            t0 = time.perf_counter()
            rc = idx.refine_chains_raw(ests, exons, q, n)[0]
            t1 = time.perf_counter()
            if rc != capi.PGPU_OK:
                raise SystemExit("chain_cost: pgpu_index_refine_chains returned %d" % rc)
            ms = idx.refine_chains_kernel_ms()
            clock = {}
            t2 = time.perf_counter()
            CL.device_rounds(ctx, idx, gen, batch, clock=clock)
            t3 = time.perf_counter()
            print("chain_cost: call %d of %d: fused %.2f ms, rounds %.0f ms" % (r + 1, a.warmup + a.repeats, 1e3 * (t1 - t0),
                                                                                  1e3 * (t3 - t2)), file=sys.stderr, flush=True)
            if r >= a.warmup:
                kern.append(ms); wall.append(1e3 * (t1 - t0)); rounds_wall.append(1e3 * (t3 - t2)); rounds_lib.append(1e3 * clock["library_s"])
        alloc = workspace_alloc_ms(a.cus, a.repeats)
        idx.close()
    print(json.dumps({"chains": n, "introns": int(res["done"].sum()), "exons": int(len(exons)), "bases": len(gen),
                      "dropped_first": int(res["dropped_first"].sum()),
                      "paths": np.bincount(out_steps[out_steps > 0] & 15, minlength=10).tolist(),
                      "fused_kernel_ms": spread(kern), "fused_call_wall_ms": spread(wall),
                      "workspace_alloc_free_ms": alloc,
                      "rounds_wall_ms": spread(rounds_wall), "rounds_inside_library_ms": spread(rounds_lib)}))


if __name__ == "__main__":
    main()
