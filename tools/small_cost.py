"""Cost of the last two routines of refine_EST_factorizations chained on the resident index (pgpu_index_small_chains) next
to the same questions by the device route that exists without it, and what a C3-shaped chunk looks like to the entry.

One process.  A batch of `--queries` generated factorizations over a seeded sequence of planted loci (tests/small_lib.py:
generated), answered
  (a) by the one fused call per min_intron_length: HIP-event time of the kernel and wall time of the whole synchronous
      call, after warm-up calls, `--repeats` times, summed over the values;
  (b) by the restatement over the CPU oracle, which records every question the three steps ask (common factor of the
      prefix, edit distance, border refinement, common factor of two exon ends, intron class, small-exon search, banded
      distance); the fused call's bytes are compared with its answers first;
  (c) by ONE round that holds all of those questions: one DP plan (PGPU_DP_LCF with PGPU_JOB_A_GENOMIC, PGPU_DP_ED,
      PGPU_DP_BORDERS with PGPU_JOB_B_GENOMIC, PGPU_DP_KBAND), one pgpu_index_classify and one pgpu_index_small_exons: the
      seconds inside the library's own entry points, `--route-repeats` times, the answers compared with the oracle's.  This is
      the baseline, and it flatters the route: a caller does not know all questions at once (the refinement needs the common
      factor and the edit distance, the search the two distances, the class and the two factors, the cleaning the list
      after both: tests/small_lib.py: device_route needs a round per dependency), and the glue between the questions is not
      in this clock.
How many queries are refused, by `refused` code, and how many questions of each kind there are, is reported for both batches.

The C3-shaped batch: the DONE factorizations of the first `--ests` ESTs of pintron_amd/synth.py's C3, both strands, as
pgpu_pairing_plan_run_factorizations and then pgpu_index_tail_chains leave them (tools/tail_cost.py's chunk, one stage
further), with min_intron_length 40.  Median and range as one JSON line."""
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


class Recorder:
    """the oracle's answers, and every question with its answer"""

    def __init__(self, SL, gen):
        self.o = SL.OracleOps(gen)
        self.first_bad = self.o.first_bad
        self.asked = {}

    def _keep(self, key, answer):
        if key not in self.asked:
            self.asked[key] = answer()
        return self.asked[key]

    def lcf_prefix(self, gstart, piece):
        return self._keep(("lcfp", gstart, piece), lambda: self.o.lcf_prefix(gstart, piece))

    def ed(self, a, b):
        return self._keep(("ed", a, b), lambda: self.o.ed(a, b))

    def borders(self, p, gstart, glen, p0, p1, max_errs):
        return self._keep(("borders", p, gstart, glen, p0, p1, max_errs), lambda: self.o.borders(p, gstart, glen, p0, p1, max_errs))

    def lcf(self, a, b):
        return self._keep(("lcf", a, b), lambda: self.o.lcf(a, b))

    def classify(self, start, end):
        return self._keep(("class", start, end), lambda: self.o.classify(start, end))

    def sexon(self, efact, allgstart, allglen, f1slen, f2plen, mil, info=None):
        return self._keep(("sexon", efact, allgstart, allglen, f1slen, f2plen, mil),
                          lambda: self.o.sexon(efact, allgstart, allglen, f1slen, f2plen, mil))

    def kband(self, g, e, ub):
        return self._keep(("kband", g, e, ub), lambda: self.o.kband(g, e, ub))


def one_round(ctx, idx, gen, asked, capi):
    """every recorded question in one plan, one classify call and one small-exon call -> seconds inside the library's
    entry points; the answers are checked"""
    kinds = {"lcfp": capi.LCF, "lcf": capi.LCF, "ed": capi.ED, "borders": capi.BORDERS, "kband": capi.KBAND}
    dp = [k for k in asked if k[0] in kinds]
    jl = capi.JobList()
    for key in dp:
        if key[0] == "lcfp":
            jl.add(capi.LCF, bytes(key[1]), key[2], a_gen_off=0)
        elif key[0] in ("lcf", "ed"):
            jl.add(kinds[key[0]], key[1], key[2])
        elif key[0] == "kband":
            jl.add(capi.KBAND, key[1], key[2], p0=key[3])
        else:
            _, p, gstart, glen, p0, p1, max_errs = key
            jl.add(capi.BORDERS, p, bytes(glen), p0=p0, p1=p1, p2=max_errs, b_gen_off=gstart, tail=min(2, len(gen) - (gstart + glen)))
    inside = 0.0
    if dp:
        t0 = time.perf_counter()
        got = capi.run_jobs(ctx, jl, idx)
        inside += time.perf_counter() - t0
        for key, o in zip(dp, got):
            want = asked[key]
            if key[0] in ("lcfp", "lcf"):
                ok = (o["len"], o["occ1"], o["occ2"]) == tuple(want)
            elif key[0] == "ed":
                ok = o["score"] == want
            elif key[0] == "kband":
                ok = bool(o["ok"]) == want
            else:
                ok = all(o[k] == want[k] for k in want)
            if o["status"] != 0 or not ok:
                raise SystemExit("small_cost: the plan's answer to %r is %r, the oracle's %r" % (key[0], o, want))
    cl = [k for k in asked if k[0] == "class"]
    if cl:
        t0 = time.perf_counter()
        got = idx.classify([k[1] for k in cl], [k[2] for k in cl])
        inside += time.perf_counter() - t0
        if [int(x) for x in got] != [asked[k] for k in cl]:
            raise SystemExit("small_cost: pgpu_index_classify and the restatement disagree")
    sx = [k for k in asked if k[0] == "sexon"]
    if sx:
        blob, rows, off = [], [], 0
        for _, efact, allgstart, allglen, f1, f2, mil in sx:
            rows.append((off, len(efact), allgstart, allglen, f1, f2, mil))
            blob.append(efact)
            off += len(efact)
        t0 = time.perf_counter()
        got = idx.small_exons(b"".join(blob), rows)
        inside += time.perf_counter() - t0
        for key, o in zip(sx, got):
            if (int(o["len"]), int(o["offstart"]), int(o["offend"]), int(o["gpos"])) != tuple(asked[key]):
                raise SystemExit("small_cost: pgpu_index_small_exons and the transcription disagree")
    return inside


def measure(ctx, idx, gen, batch, a, SL, capi):
    rec = Recorder(SL, gen)
    infos = [{} for _ in batch]
    want = [SL.small(o, e, gen, ex, mil, ops=rec, info=i) for (_, o, e, ex, mil), i in zip(batch, infos)]
    groups = []
    for mil in sorted({c[4] for c in batch}):
        part = [(c, w) for c, w in zip(batch, want) if c[4] == mil]
        ests, exons, q = SL.batch_arrays([c for c, _ in part])
        rc, out_exons, out_steps, res = idx.small_chains_raw(ests, exons, q, len(q), mil)
        if rc != capi.PGPU_OK:
            raise SystemExit("small_cost: pgpu_index_small_chains returned %d" % rc)
        we, ws, wr = SL.expect_arrays(exons, q, [w for _, w in part])
        if (we.tobytes(), ws.tobytes(), wr.tobytes()) != (out_exons.tobytes(), out_steps.tobytes(), res.tobytes()):
            bad = [i for i in range(len(q)) if res[i] != wr[i]]
            raise SystemExit("small_cost: the fused call and the restatement disagree (first result: %r)" % (bad[:1],))
        groups.append((mil, ests, exons, q))
    n = len(batch)
    print("small_cost: %d answers equal the restatement's" % n, file=sys.stderr, flush=True)
    kern, wall = [], []
    for r in range(a.warmup + a.repeats):
        k = w = 0.0
        for mil, ests, exons, q in groups:
            t0 = time.perf_counter()
            rc = idx.small_chains_raw(ests, exons, q, len(q), mil)[0]
            w += 1e3 * (time.perf_counter() - t0)
            if rc != capi.PGPU_OK:
                raise SystemExit("small_cost: pgpu_index_small_chains returned %d" % rc)
            k += idx.small_chains_kernel_ms()
        if r >= a.warmup:
            kern.append(k); wall.append(w)
    by_code = {}
    for w in want:
        if w[0] != SL.OK:
            by_code[str(w[1])] = by_code.get(str(w[1]), 0) + 1
    questions = {}
    for key in rec.asked:
        questions[key[0]] = questions.get(key[0], 0) + 1
    out = {"queries": n, "calls": len(groups), "exons": sum(len(c[3]) for c in batch), "est_bytes": sum(len(g[1]) for g in groups),
           "refused": sum(by_code.values()), "refused_by_code": by_code,
           "prefix_added": sum(w[3] for w in want), "queries_with_an_exon_between": sum(w[4] - w[3] > 0 for w in want),
           "exons_added": sum(w[4] for w in want), "queries_step3_drops_from": sum(w[0] == SL.OK and w[7] < w[5] for w in want),
           "emptied": sum(w[2] != 0 for w in want),
           "asked": {k: sum(i.get("dp_" + k, 0) for i in infos) for k in ("lcf", "ed", "borders", "lcf_small", "class", "sexon", "kband")},
           "distinct_questions": questions,
           "fused_kernel_ms": spread(kern), "fused_call_wall_ms": spread(wall)}
    if rec.asked:
        out["one_round_inside_library_ms"] = spread([1e3 * one_round(ctx, idx, gen, rec.asked, capi) for _ in range(a.route_repeats)])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=100_000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--route-repeats", type=int, default=3)
    ap.add_argument("--ests", type=int, default=10_000, help="ESTs of the C3-shaped chunk (0: leave it out)")
    a = ap.parse_args()
    import small_lib as SL
    import tail_lib as TL
    from pintron_amd import capi
    out = {}
    with capi.Context(0) as ctx:
        gen, batch = SL.generated(43, a.queries)
        idx = capi.Index(ctx, gen)
        out["generated"] = dict(measure(ctx, idx, gen, batch, a, SL, capi), bases=len(gen))
        idx.close()
        if a.ests:
            import fact_lib as F
            import pairing_lib as PL
            from pintron_amd import synth
            w = synth.make("C3", n_est=a.ests)
            seqs = list(w.est_seqs) + [PL.revcomp(e) for e in w.est_seqs]
            genomic = bytes(w.genomic)
            idx = capi.Index(ctx, genomic)
            plan = capi.PairingPlan(ctx, idx, seqs, resident=True)
            plan.run(15, 0.2)
            plan.run_meg()
            plan.run_candidates(15, 40)
            plan.run_factorizations(*F.DEFAULTS)
            res, exons, steps = plan.fetch_factorizations()
            plan.close()
            tail_in = []
            for i in np.flatnonzero(res["outcome"] == F.DONE):
                lo, k = int(res[i]["first_exon"]), int(res[i]["n_exons"])
                ex = [tuple(int(v) for v in e) for e in exons[lo:lo + k]]
                est = bytes(seqs[i])
                if not TL.einval(len(est), len(genomic), ex, [dict(est_off=0, est_len=len(est), first_exon=0, n_exons=k, reserved=0, orig_off=0)]):
                    tail_in.append(("c3", est, est, ex))
            ests_t, exons_t, q_t = TL.batch_arrays(tail_in)
            oe, os_, tr = idx.tail_chains(ests_t, exons_t, q_t)
            batch, tail_refused, tail_dropped = [], 0, 0
            for i, c in enumerate(tail_in):
                if tr[i]["status"] != 0:
                    tail_refused += 1
                    continue
                if tr[i]["verdict"] != 0:
                    tail_dropped += 1
                    continue
                lo, k = int(q_t[i]["first_exon"]), int(q_t[i]["n_exons"])
                ex = [tuple(int(v) for v in e) for e, s in zip(oe[lo:lo + k], os_[lo:lo + k]) if s & 3 != TL.REMOVED]
                batch.append(("c3", c[1], c[2], ex, 40))
            out["c3_shaped"] = dict(measure(ctx, idx, genomic, batch, a, SL, capi), patterns=len(seqs),
                                    done=int((res["outcome"] == F.DONE).sum()), refused_by_the_tail_stage=tail_refused,
                                    dropped_by_the_tail_stage=tail_dropped, bases=len(genomic))
            idx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
