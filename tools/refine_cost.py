"""Cost of the intron-border decision on the resident index (pgpu_index_refine_introns) next to the same work on the host.

One batch of 100 000 queries on a random 200 kb sequence: 12 500 generated introns (tests/refine_lib.py: planted sites of
every kind, moved borders, errors near the junction), each with its gap alignment from the oracle and under eight
settings (first / later intron, four min_intron_length), answered (a) by the library: HIP-event time of the kernel and
wall time of the whole synchronous call; (b) on one host thread by the product's own host code with a CPU edit
distance (tools/exp/refine_host.c, which includes pintron_amd/host/ef_refine_intron.c), compiled here into a temporary
directory.  The answers are compared first; warm-up calls, then `--repeats` timed ones, the two paths alternating;
median and range as one JSON line."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4), "n": len(xs)}


def workload(bases, distinct, seed):
    import oracle_lib as O
    import refine_lib as RL
    rng = np.random.default_rng(seed)
    g = bytearray(RL.rnd(rng, bases))
    plans = [RL.make_case(rng, int(rng.integers(200, bases - 1500))) for _ in range(distinct)]
    for c in plans:
        for pos, s in c["edits"]:
            g[pos:pos + len(s)] = s
    gen = bytes(g)
    items = []
    for c in plans:
        case = None
        while case is None:
            case = RL.finish_case(rng, gen, c)
        est, donor, acceptor, _, st = case
        er, gr, v = RL.oracle_rows(O, est, gen, donor, acceptor, *st[:3])
        ilen = acceptor[2] - donor[3] - 1
        for first in (False, True):
            for mil in (4, 40, ilen, ilen + 25):
                items.append((est + b"\0", er, gr, v, donor, acceptor, first, st[:3] + (mil,)))
    ests, rows, q = RL.query_array(items)
    q["est_len"] -= 1                                     # the host code wants its ESTs terminated; the library gets the length
    return gen, ests, rows, q


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=100_000)
    ap.add_argument("--bases", type=int, default=200_000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=9)
    a = ap.parse_args()
    from pintron_amd import capi
    gen, ests, rows, q = workload(a.bases, a.queries // 8, seed=31)
    n = len(q)
    with tempfile.TemporaryDirectory() as d:
        so = os.path.join(d, "refine_host.so")
        subprocess.run(["gcc", "-O2", "-fPIC", "-shared", "-o", so, os.path.join(ROOT, "tools", "exp", "refine_host.c")], check=True)
        H = C.CDLL(so)
        H.refine_host_batch.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_void_p, C.c_size_t, C.c_void_p]
        H.refine_host_batch.restype = None
        gbuf = C.create_string_buffer(gen)                    # NUL-terminated, alive for the whole run
        want = np.zeros(n, dtype=np.dtype(capi.REFINE_RESULT_DTYPE))

        def host():
            H.refine_host_batch(gbuf, ests, rows, q.ctypes.data, n, want.ctypes.data)
        host()
        with capi.Context(0) as ctx:
            idx = capi.Index(ctx, gen)
            rc, got = idx.refine_introns_raw(ests, rows, q, n)
            if rc != capi.PGPU_OK:
                raise SystemExit("refine_cost: pgpu_index_refine_introns returned %d" % rc)
            if got.tobytes() != want.tobytes():
                bad = [i for i in range(n) if got[i] != want[i]]
                raise SystemExit("refine_cost: the library and the host code disagree on %d queries (first: %d: %r / %r)"
                                 % (len(bad), bad[0], got[bad[0]], want[bad[0]]))
            kern, wall, host_ms = [], [], []
            for r in range(a.warmup + a.repeats):             # the two paths alternate: they see the same machine
                t0 = time.perf_counter()
                rc, got = idx.refine_introns_raw(ests, rows, q, n)
                t1 = time.perf_counter()
                if rc != capi.PGPU_OK:
                    raise SystemExit("refine_cost: pgpu_index_refine_introns returned %d" % rc)
                ms = idx.refine_introns_kernel_ms()
                t2 = time.perf_counter()
                host()
                t3 = time.perf_counter()
                if r >= a.warmup:
                    kern.append(ms); wall.append(1e3 * (t1 - t0)); host_ms.append(1e3 * (t3 - t2))
            idx.close()
    print(json.dumps({"queries": n, "bases": len(gen), "refined": int(want["refined"].sum()),
                      "paths": np.bincount(want["path"], minlength=10).tolist(),
                      "gpu_kernel_ms": spread(kern), "gpu_call_wall_ms": spread(wall), "host_one_thread_ms": spread(host_ms)}))


if __name__ == "__main__":
    main()
