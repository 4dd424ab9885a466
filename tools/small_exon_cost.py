"""Cost of the small-exon search on the resident index (pgpu_index_small_exons) next to the same work on the host.

One batch of 100 000 queries on a random 200 kb sequence with planted small exons (tests/small_exon_lib.py: introns of
500 bp - 20 kb, small exons of 6..30, EST factors with and without errors) answered (a) by the library: HIP-event time
of the kernel, wall time of the whole synchronous call, and the one-off build of the index's classification tables
(the first call on a fresh index against the next one); (b) on one host thread by the transcription's algorithm in C
(tools/exp/small_exon_host.c: two loops, memmem, the product's ef_classify.c with its tables prepared beforehand),
compiled here into a temporary directory.  The answers are compared first; warm-up calls, then `--repeats` timed
ones, the two paths alternating; median and range as one JSON line."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=100_000)
    ap.add_argument("--bases", type=int, default=200_000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=9)
    a = ap.parse_args()
    import small_exon_lib as SL
    from pintron_amd import capi
    gen, loci = SL.planted_genomic(a.bases, seed=21)
    ests, q = SL.planted_queries(gen, loci, a.queries, seed=23)
    n = len(q)
    fields = ("status", "len", "offstart", "offend", "gpos", "i1type", "i2type")

    with tempfile.TemporaryDirectory() as d:
        so = os.path.join(d, "small_exon_host.so")
        subprocess.run(["gcc", "-O2", "-fPIC", "-shared", "-pthread", "-o", so, os.path.join(ROOT, "tools", "exp", "small_exon_host.c"),
                        os.path.join(ROOT, "pintron_amd", "host", "ef_classify.c"), "-lm"], check=True)
        H = C.CDLL(so)
        H.sexon_host_prepare.argtypes = [C.c_char_p]
        H.sexon_host_batch.argtypes = [C.c_char_p, C.c_void_p, C.c_size_t, C.c_void_p]
        H.sexon_host_prepare.restype = H.sexon_host_batch.restype = None
        gbuf = C.create_string_buffer(gen)                   # NUL-terminated, alive for the whole run
        t0 = time.perf_counter()
        H.sexon_host_prepare(gbuf)
        host_prepare_ms = 1e3 * (time.perf_counter() - t0)
        want = np.zeros(n, dtype=np.dtype(capi.SEXON_RESULT_DTYPE))

        def host():
            H.sexon_host_batch(ests, q.ctypes.data, n, want.ctypes.data)
        host()
        with capi.Context(0) as ctx:
            idx = capi.Index(ctx, gen)
            t0 = time.perf_counter()
            idx.classify([100], [200])                       # first use: builds the tables
            t1 = time.perf_counter()
            idx.classify([100], [200])
            t2 = time.perf_counter()
            tables_ms = 1e3 * ((t1 - t0) - (t2 - t1))
            rc, got = idx.small_exons_raw(ests, q, n)
            if rc != capi.PGPU_OK:
                raise SystemExit("small_exon_cost: pgpu_index_small_exons returned %d" % rc)
            for f in fields:
                if not np.array_equal(got[f], want[f]):
                    bad = np.nonzero(got[f] != want[f])[0]
                    raise SystemExit("small_exon_cost: the library and the host loop disagree on %r in %d queries (first: %d: %r / %r)"
                                     % (f, len(bad), bad[0], got[bad[0]], want[bad[0]]))
            kern, wall, host_ms = [], [], []
            for r in range(a.warmup + a.repeats):            # the two paths alternate: they see the same machine
                t0 = time.perf_counter()
                rc, got = idx.small_exons_raw(ests, q, n)
                t1 = time.perf_counter()
                if rc != capi.PGPU_OK:
                    raise SystemExit("small_exon_cost: pgpu_index_small_exons returned %d" % rc)
                ms = idx.small_exons_kernel_ms()
                t2 = time.perf_counter()
                host()
                t3 = time.perf_counter()
                if r >= a.warmup:
                    kern.append(ms); wall.append(1e3 * (t1 - t0)); host_ms.append(1e3 * (t3 - t2))
            idx.close()
    print(json.dumps({"queries": n, "bases": len(gen), "found": int((want["len"] > 0).sum()),
                      "gpu_kernel_ms": spread(kern), "gpu_call_wall_ms": spread(wall), "gpu_class_tables_once_ms": round(tables_ms, 3),
                      "host_one_thread_ms": spread(host_ms), "host_tables_once_ms": round(host_prepare_ms, 3)}))


if __name__ == "__main__":
    main()
