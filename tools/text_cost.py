"""Cost of the text stage (pgpu_pairing_plan_run_texts) on a C3-shaped chunk: the first `--ests` ESTs of
pintron_amd/synth.py's C3 (200 kb, ESTs of 600 +- 100 bases with 3 % errors), both strands -- the chunk of tools/unit_cost.py:
2 x ests patterns, ests units, unit k = (pattern k, pattern ests + k), a header of about 30 bytes per unit.

One resident plan, one process.  The ladder runs once up to the units; then, after warm-up rounds, `--repeats` rounds of
run_texts + fetch_texts into page-locked buffers on the host clock (what a caller waits for) and
pgpu_pairing_plan_texts_ms, the HIP-event time of count + scans + write.  The first round's answer is compared with the
restatement (tests/text_lib.py) on the fetched units, every later round's with the first.

For comparison, the host's own routines over the same records in one thread (tools/text_cost_host.c, compiled here against
pintron_amd/lib/libestfact.so): ef_raw_text_from_records plus ef_write_single_est_info per EST, in CPU time.  That is the
product's code and the yardstick.  One JSON line, printed and, with --out, written to that file (profiles/text_cost.txt is
such a file; DESIGN.md section 5p is copied from it by hand)."""
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


def host_routine(d, genomic, rec, raw, pests, repeats):
    """[(raw ms, pests ms)] of tools/text_cost_host.c over the given records; it checks both texts against the device's"""
    exe = os.path.join(d, "text_cost_host")
    lib = os.path.join(ROOT, "pintron_amd", "lib")
    subprocess.run(["gcc", "-std=gnu99", "-O2", "-o", exe, os.path.join(ROOT, "tools", "text_cost_host.c"), "-L" + lib, "-lestfact",
                    "-Wl,-rpath," + lib, "-Wl,-rpath-link,/opt/rocm/lib", "-lm", "-pthread"], check=True)
    for name, data in (("genomic", genomic), ("records.bin", rec), ("pests.txt", pests), ("raw.txt", raw)):
        with open(os.path.join(d, name), "wb") as f:
            f.write(data)
    r = subprocess.run([exe, "genomic", "records.bin", "pests.txt", "raw.txt", str(repeats)], cwd=d, check=True, capture_output=True, text=True)
    return [tuple(float(x) for x in ln.split()) for ln in r.stdout.splitlines()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ests", type=int, default=10_000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    import fact_lib as F
    import pairing_lib as PL
    import text_lib as TL
    import unit_lib as UL
    from pintron_amd import capi, synth
    w = synth.make("C3", n_est=a.ests)
    n = len(w.est_seqs)
    seqs = list(w.est_seqs) + [PL.revcomp(e) for e in w.est_seqs]
    q = UL.query_array([(k, k, n + k, 0) for k in range(n)])
    headers = [b"/gb=EST%07d /gi=%d /len=%d" % (k, 1000000 + k, len(w.est_seqs[k])) for k in range(n)]
    hb, hf = capi._offsets(headers)
    out = {"patterns": len(seqs), "units": n, "bases": len(w.genomic), "header_bytes": len(hb)}
    ms, write_ms, wall = [], [], []
    first = None
    with capi.Context(0) as ctx:
        L = ctx.L
        idx = capi.Index(ctx, w.genomic)
        src = capi.TextSource(ctx, w.genomic)
        plan = capi.PairingPlan(ctx, idx, seqs, resident=True)
        plan.run(15, 0.2)
        plan.run_meg()
        plan.run_candidates(15, 40)
        plan.run_factorizations(*F.DEFAULTS)
        plan.run_final_factorizations(40)
        plan.run_units(q, 0, True)
        units, blob = plan.fetch_units()
        ctx.check(plan.run_texts_raw(src, hb, len(hb), hf))
        raw_n, pests_n = plan.text_bytes(0), plan.text_bytes(1)
        res = np.zeros(n, dtype=np.dtype(capi.TEXT_RESULT_DTYPE))
        pinned = [C.c_void_p(), C.c_void_p()]
        for p, size in zip(pinned, (raw_n, pests_n)):
            ctx.check(L.pgpu_host_alloc(ctx.h, max(size, 1), C.byref(p)))
        for r in range(a.warmup + a.repeats):
            t0 = time.perf_counter()
            ctx.check(plan.run_texts_raw(src, hb, len(hb), hf))
            ctx.check(L.pgpu_pairing_plan_fetch_texts(ctx.h, plan.h, res.ctypes.data_as(C.POINTER(capi.TextResult)), pinned[0], raw_n,
                                                      pinned[1], pests_n))
            t1 = time.perf_counter()
            got = (res.tobytes(), C.string_at(pinned[0], raw_n), C.string_at(pinned[1], pests_n))
            if first is None:
                want = TL.texts(units, blob, headers, seqs, w.genomic)
                if want[0].tobytes() != got[0] or want[1] != got[1] or want[2] != got[2]:
                    raise SystemExit("text_cost: the device and the restatement disagree")
                first = got
            elif got != first:
                raise SystemExit("text_cost: a rerun gave other bytes")
            if r >= a.warmup:
                ms.append(plan.texts_ms())
                write_ms.append(plan.texts_write_ms())
                wall.append(1e3 * (t1 - t0))
        for p in pinned:
            L.pgpu_host_free(ctx.h, p)
        v = res["verdict"]
        # the host routine over the records of the DONE units alone: the same ESTs, the same bytes
        done = v == TL.DONE
        rec = b"".join(blob[int(a_):int(a_) + int(n_)] for a_, n_ in zip(units["first_byte"][done], units["n_bytes"][done]))
        with tempfile.TemporaryDirectory() as d:
            host = host_routine(d, w.genomic, rec, first[1], first[2], a.warmup + a.repeats)[a.warmup:]
        host_ms = [x + y for x, y in host]
        kernel = statistics.median(write_ms)
        out.update(verdicts={"done": int(done.sum()), "none": int((v == TL.NONE).sum()), "host": int((v == TL.HOST).sum())},
                   raw_bytes=raw_n, pests_bytes=pests_n, record_bytes=len(rec),
                   texts_ms=spread(ms), write_pass_ms=spread(write_ms), run_texts_and_fetch_wall_ms=spread(wall),
                   write_pass_gb_per_s_written=round((raw_n + pests_n) / (kernel * 1e6), 3) if kernel > 0 else None,
                   host_raw_text_from_records_cpu_ms=spread([x for x, _ in host]), host_processed_ests_cpu_ms=spread([y for _, y in host]),
                   host_both_cpu_ms=spread(host_ms),
                   device_wall_over_host_cpu=round(statistics.median(wall) / statistics.median(host_ms), 4))
        plan.close()
        src.close()
        idx.close()
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
