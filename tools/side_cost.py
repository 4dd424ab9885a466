"""Cost of the side stage (pgpu_pairing_plan_run_sides) on a C3-shaped chunk: the first `--ests` ESTs of
pintron_amd/synth.py's C3 (200 kb, ESTs of 600 +- 100 bases with 3 % errors), both strands -- the chunk of tools/unit_cost.py
and tools/text_cost.py: 2 x ests patterns, ests units, unit k = (pattern k, pattern ests + k), a header of about 30 bytes per
unit.

One resident plan, one process.  The ladder runs once up to the texts; then, after warm-up rounds, `--repeats` rounds of
run_sides + fetch_sides into page-locked buffers on the host clock (what a caller waits for), pgpu_pairing_plan_sides_ms,
the HIP-event time of count + scans + write, and pgpu_pairing_plan_sides_write_ms, the write pass alone.  The first round's
answer is compared with the restatement (tests/side_lib.py) on the fetched records and units, every later round's with the
first.  One more figure the wiring needs: the bytes of fetch_meg for the whole chunk against the bytes of the records that
only the HOST units' patterns name.

For comparison, the host's own code over the same records for the same settled units in one thread
(tools/side_cost_host.c, compiled here against pintron_amd/lib/libestfact.so), in CPU time.  That is the product's code and
the yardstick.  One JSON line, printed and, with --out, written to that file (profiles/side_cost.txt is such a file;
DESIGN.md section 5q is copied from it by hand)."""
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


def host_routine(d, records, q, units, headers, seqs, blobs, repeats):
    """[ms] of tools/side_cost_host.c over the settled units; it checks the three texts against the device's"""
    from pintron_amd import capi
    exe = os.path.join(d, "side_cost_host")
    lib = os.path.join(ROOT, "pintron_amd", "lib")
    subprocess.run(["gcc", "-std=gnu99", "-O2", "-o", exe, os.path.join(ROOT, "tools", "side_cost_host.c"), "-L" + lib, "-lestfact",
                    "-Wl,-rpath," + lib, "-Wl,-rpath-link,/opt/rocm/lib", "-lm", "-pthread"], check=True)
    rb, rf = capi._offsets(records)
    table = np.array([(int(u["verdict"]) == 2, int(u["strand"]), int(x["fwd"]), int(x["rev"])) for x, u in zip(q, units)], dtype="<u4")
    files = (("recs.bin", rb), ("rec_first.bin", rf.astype("<u8").tobytes()), ("units.bin", table.tobytes()),
             ("headers.txt", b"".join(h + b"\n" for h in headers)), ("seqs.txt", b"".join(s + b"\n" for s in seqs)),
             ("megs", blobs[0]), ("pmegs", blobs[1]), ("edges", blobs[2]))
    for name, data in files:
        with open(os.path.join(d, name), "wb") as f:
            f.write(data)
    r = subprocess.run([exe] + [name for name, _ in files] + [str(repeats)], cwd=d, check=True, capture_output=True, text=True)
    return [float(ln) for ln in r.stdout.splitlines()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ests", type=int, default=10_000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    import fact_lib as F
    import pairing_lib as PL
    import side_lib as SL
    import unit_lib as UL
    from pintron_amd import capi, synth
    w = synth.make("C3", n_est=a.ests)
    n = len(w.est_seqs)
    seqs = list(w.est_seqs) + [PL.revcomp(e) for e in w.est_seqs]
    q = UL.query_array([(k, k, n + k, 0) for k in range(n)])
    headers = [b"/gb=EST%07d /gi=%d /len=%d" % (k, 1000000 + k, len(w.est_seqs[k])) for k in range(n)]
    out = {"patterns": len(seqs), "units": n, "bases": len(w.genomic), "header_bytes": sum(len(h) for h in headers)}
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
        units, _ = plan.fetch_units()
        records = plan.fetch_meg()
        plan.run_texts(src, headers)
        sizes = plan.run_sides()
        res = np.zeros(n, dtype=np.dtype(capi.SIDE_RESULT_DTYPE))
        pinned = [C.c_void_p(), C.c_void_p(), C.c_void_p()]
        for p, size in zip(pinned, sizes):
            ctx.check(L.pgpu_host_alloc(ctx.h, max(size, 1), C.byref(p)))
        for r in range(a.warmup + a.repeats):
            t0 = time.perf_counter()
            ctx.check(plan.run_sides_raw())
            ctx.check(L.pgpu_pairing_plan_fetch_sides(ctx.h, plan.h, res.ctypes.data_as(C.POINTER(capi.SideResult)), pinned[0], sizes[0],
                                                      pinned[1], sizes[1], pinned[2], sizes[2]))
            t1 = time.perf_counter()
            got = (res.tobytes(),) + tuple(C.string_at(p, size) for p, size in zip(pinned, sizes))
            if first is None:
                want = SL.sides(q, units, records, headers, seqs)
                if want[0].tobytes() != got[0] or want[1:] != got[1:]:
                    raise SystemExit("side_cost: the device and the restatement disagree")
                first = got
            elif got != first:
                raise SystemExit("side_cost: a rerun gave other bytes")
            if r >= a.warmup:
                ms.append(plan.sides_ms())
                write_ms.append(plan.sides_write_ms())
                wall.append(1e3 * (t1 - t0))
        for p in pinned:
            L.pgpu_host_free(ctx.h, p)
        v = res["verdict"]
        done = np.nonzero(v == SL.DONE)[0]
        assert not (v == SL.HOST).any()                 # every settled unit is DONE: the host routine prints the same units
        with tempfile.TemporaryDirectory() as d:
            host_ms = host_routine(d, records, q[done], units[done], [headers[i] for i in done], seqs, first[1:], a.warmup + a.repeats)[a.warmup:]
        # what the wiring still has to fetch: the records of the patterns of the HOST units
        host_units = np.nonzero(units["verdict"] == UL.U_HOST)[0]
        host_pats = set(int(x) for i in host_units for x in (q["fwd"][i], q["rev"][i]) if int(x) != UL.NO_SIBLING)
        kernel = statistics.median(write_ms)
        out.update(verdicts={"done": int(len(done)), "none": int((v == SL.NONE).sum()), "host": int((v == SL.HOST).sum())},
                   units_aligned=int((units["verdict"] == UL.U_ALIGNED).sum()), units_unaligned=int((units["verdict"] == UL.U_UNALIGNED).sum()),
                   units_on_the_sibling=int(((units["verdict"] != UL.U_HOST) & (units["strand"] == 1)).sum()),
                   megs_bytes=sizes[0], pmegs_bytes=sizes[1], edges_bytes=sizes[2],
                   sides_ms=spread(ms), write_pass_ms=spread(write_ms), run_sides_and_fetch_wall_ms=spread(wall),
                   write_pass_gb_per_s_written=round(sum(sizes) / (kernel * 1e6), 3) if kernel > 0 else None,
                   host_side_files_cpu_ms=spread(host_ms),
                   device_wall_over_host_cpu=round(statistics.median(wall) / statistics.median(host_ms), 4),
                   fetch_meg_bytes=sum(len(r) for r in records), host_units_record_bytes=sum(len(records[x]) for x in host_pats))
        plan.close()
        src.close()
        idx.close()
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
