"""Cost of the exact-occurrence query (pgpu_index_find) next to the host path it would replace.

One batch of 100 000 queries on a random 200 kb sequence -- patterns of 6-12 bytes, windows of 500 bp - 20 kb, the
intron sizes synth.py plants -- answered (a) by the library: HIP-event time of the count + scan and of the fill
kernels and the wall time of the whole synchronous call, and (b) by memmem() in a loop on one host thread
(tools/exp/find_memmem.c, compiled here into a temporary directory).  Warm-up calls first, then `--repeats`
timed ones; median and range are printed as one JSON line.  The two answers are compared before anything is timed."""
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


def batch(gen, n_queries, seed):
    rng = np.random.default_rng(seed)
    n = len(gen)
    lens = rng.integers(6, 13, size=n_queries)
    at = rng.integers(0, n - 12, size=n_queries)
    width = rng.integers(500, 20_001, size=n_queries)
    lo = np.maximum(0, at - (rng.random(n_queries) * width).astype(np.int64))
    hi = np.minimum(n, lo + width)
    return [gen[a:a + m] for a, m in zip(at.tolist(), lens.tolist())], list(zip(lo.tolist(), hi.tolist()))


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4), "n": len(xs)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=100_000)
    ap.add_argument("--bases", type=int, default=200_000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=9)
    a = ap.parse_args()
    from pintron_amd import capi
    gen = np.random.default_rng(3).choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=a.bases).tobytes()
    pats, wins = batch(gen, a.queries, seed=8)
    blob = b"".join(pats)
    lens = np.array([len(p) for p in pats], dtype=np.uint32)
    off = np.zeros(len(pats), dtype=np.uint64)
    off[1:] = np.cumsum(lens[:-1])
    lo = np.array([w[0] for w in wins], dtype=np.uint32)
    hi = np.array([w[1] for w in wins], dtype=np.uint32)

    with tempfile.TemporaryDirectory() as d:
        so = os.path.join(d, "find_memmem.so")
        subprocess.run(["gcc", "-O2", "-fPIC", "-shared", "-o", so, os.path.join(ROOT, "tools", "exp", "find_memmem.c")], check=True)
        H = C.CDLL(so)
        H.find_memmem_batch.restype = C.c_size_t
        H.find_memmem_batch.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_size_t, C.c_void_p, C.c_size_t]

        def host(out):
            return H.find_memmem_batch(gen, len(gen), blob, off.ctypes.data, lens.ctypes.data, lo.ctypes.data, hi.ctypes.data,
                                       len(pats), out.ctypes.data, len(out))
        total = host(np.zeros(1, dtype=np.uint32))
        want = np.zeros(total, dtype=np.uint32)
        host(want)
        with capi.Context(0) as ctx:
            idx = capi.Index(ctx, gen)
            got = idx.find(pats, wins)
            flat = np.concatenate(got) if got else np.zeros(0, dtype=np.uint32)
            if not np.array_equal(flat, want):
                raise SystemExit("find_cost: the library and memmem disagree")
            q = (capi.FindQuery * len(pats))()
            for i in range(len(pats)):
                q[i] = capi.FindQuery(int(off[i]), int(lens[i]), 0, int(lo[i]), int(hi[i]))
            out = np.zeros(total, dtype=np.uint32)
            k_count, k_fill, wall, host_ms = [], [], [], []
            for r in range(a.warmup + a.repeats):          # the two paths alternate: they see the same machine
                t0 = time.perf_counter()
                rc, _, _ = idx.find_raw(blob, q, len(pats), out)
                t1 = time.perf_counter()
                if rc != capi.PGPU_OK:
                    raise SystemExit("find_cost: pgpu_index_find returned %d" % rc)
                ms = idx.find_kernel_ms()
                t2 = time.perf_counter()
                host(want)
                t3 = time.perf_counter()
                if r >= a.warmup:
                    k_count.append(ms["count+scan"]); k_fill.append(ms["fill"])
                    wall.append(1e3 * (t1 - t0)); host_ms.append(1e3 * (t3 - t2))
            idx.close()
    print(json.dumps({"queries": len(pats), "bases": len(gen), "occurrences": int(total),
                      "gpu_count_scan_ms": spread(k_count), "gpu_fill_ms": spread(k_fill), "gpu_call_wall_ms": spread(wall),
                      "host_memmem_ms": spread(host_ms)}))


if __name__ == "__main__":
    main()
