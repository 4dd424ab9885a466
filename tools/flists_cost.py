"""Cost of the list stage (pgpu_pairing_plan_run_factorization_lists, pgpu_index_factorization_lists) on a C3-shaped chunk: the
first `--ests` ESTs of pintron_amd/synth.py's C3 (200 kb, ESTs of 600 +- 100 bases with 3 % errors), both strands, i.e. one
of the ten chunks a C3 step of 100 000 ESTs is prefetched in.

One resident plan, one process.  After warm-up rounds, `--repeats` rounds of run -> run_meg -> run_candidate_lists, then
  (a) pgpu_pairing_plan_factorization_lists_ms(k)          HIP-event times: the whole call, clean_kernel, flist_select_kernel,
                                                            gaps_kernel, chain_kernel;
  (b) run_factorization_lists + fetch_factorization_lists  the two calls on the host clock: what a caller waits for;
  (c) pgpu_index_factorization_lists                       on the same lists, fetched: its device part (HIP events) and the whole
                                                            call on the host clock, the uploads included;
  (d) ef_chain_factorizations                              the host code over the same fetched records on one core, once.
The plan form's answer is compared with the index form's, and on every record the device answers (DONE or EMPTY) with the
host code's.  What the chunk's records get: DONE / EMPTY / HOST per stage, over all patterns and over the branching ones
(the candidate stage says NOT_PATH and the record has more than two vertices), the units (an EST's two strands) neither of
whose strands is HOST and the units answered the way est-fact asks (the forward strand DONE, or EMPTY and the reverse one
not HOST), and the largest list.  Median and range as one JSON line."""
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


def outcomes(res, mask=None):
    r = res if mask is None else res[mask]
    out = {}
    for name, code in (("done", 2), ("empty", 1), ("host", 0)):
        for stage in range(5):
            n = int(((r["outcome"] == code) & (r["stage"] == stage)).sum())
            if n:
                out["%s_%d" % (name, stage)] = n
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ests", type=int, default=10_000)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    import cand_lib as CL
    import enum_lib as EL
    import flists_lib as F
    import pairing_lib as PL
    from pintron_amd import capi, synth
    w = synth.make("C3", n_est=a.ests)
    seqs = list(w.est_seqs) + [PL.revcomp(e) for e in w.est_seqs]
    n_pat = len(seqs)
    out = {"patterns": n_pat, "bases": len(w.genomic)}
    ms = [[] for _ in range(5)]
    wall, ix_dev, ix_wall = [], [], []
    prm = F.capi_params(F.DEFAULTS)
    off = np.zeros(n_pat + 1, dtype=np.uint64)
    np.cumsum([len(s) for s in seqs], out=off[1:])
    blob = b"".join(seqs)
    with capi.Context(0) as ctx:
        idx = capi.Index(ctx, w.genomic)
        plan = capi.PairingPlan(ctx, idx, seqs, resident=True)
        for r in range(a.warmup + a.repeats):
            plan.run(15, 0.2)
            plan.run_meg()
            plan.run_candidate_lists(15, 40)
            t0 = time.perf_counter()
            plan.run_factorization_lists(prm)
            got = plan.fetch_factorization_lists()
            t1 = time.perf_counter()
            lres, cands, exons = plan.fetch_candidate_lists()
            q = np.zeros(n_pat, dtype=np.dtype(capi.FLIST_QUERY_DTYPE))
            q["est_off"], q["est_len"] = off[:-1], np.diff(off)
            is_lists = lres["kind"] == EL.LISTS
            q["first_candidate"] = np.where(is_lists, lres["first_candidate"], 0)
            q["n_candidates"] = np.where(is_lists, lres["n_candidates"], 0)
            t2 = time.perf_counter()
            rc, res2, facts2, ex2, st2, nf, ne = idx.factorization_lists_raw(blob, cands, exons, q, n_pat, prm, len(got[1]), len(got[2]))
            t3 = time.perf_counter()
            same = is_lists | (got[0]["outcome"] == F.HOST)           # (the index form knows no enumeration kind)
            if (rc != capi.PGPU_OK or res2[is_lists].tobytes() != got[0][is_lists].tobytes() or not same.all()
                    or facts2[:nf].tobytes() != got[1].tobytes() or ex2[:ne].tobytes() != got[2].tobytes() or st2[:ne].tobytes() != got[3].tobytes()):
                raise SystemExit("flists_cost: the plan form and the index form disagree (rc %d)" % rc)
            if r >= a.warmup:
                for k in range(5):
                    ms[k].append(plan.factorization_lists_ms(k))
                wall.append(1e3 * (t1 - t0)); ix_dev.append(idx.factorization_lists_kernel_ms()); ix_wall.append(1e3 * (t3 - t2))
        recs = plan.fetch_meg()
        plan.run_candidates(15, 40)
        cres, _ = plan.fetch_candidates()
        plan.close()
        idx.close()
    res, facts, fex, fst = got
    # the yardstick: the host code over the same records, one core
    host = F.Host(w.genomic)
    host.factorizations(recs[0], seqs[0])                                   # (the library is loaded and bound outside the clock)
    t0 = time.perf_counter()
    answers = [host.factorizations(r, s) for r, s in zip(recs, seqs)]
    host_ms = 1e3 * (time.perf_counter() - t0)
    host.close()
    differ = 0
    for k, (kind, lists) in enumerate(answers):
        r = res[k]
        if int(r["outcome"]) == F.HOST:
            continue
        mine = [[tuple(int(v) for v in e) for e in fex[int(f["first_exon"]):int(f["first_exon"]) + int(f["n_exons"])].tolist()]
                for f in facts[int(r["first_fact"]):int(r["first_fact"]) + int(r["n_facts"])]]
        differ += not ((int(r["outcome"]) == F.EMPTY and kind in (0, 1)) or (int(r["outcome"]) == F.DONE and kind == 2 and lists == mine))
    if differ:
        raise SystemExit("flists_cost: the device and ef_chain_factorizations differ on %d records" % differ)
    branching = np.array([cres["kind"][k] == CL.NOT_PATH and len(CL.parse(recs[k])[1]) > 2 for k in range(n_pat)], dtype=bool)
    half = n_pat // 2
    unit_branching = branching[:half] | branching[half:]
    unit_host = (res["outcome"][:half] == F.HOST) | (res["outcome"][half:] == F.HOST)
    # est-fact takes the forward strand first and its reverse complement only when the forward one has no factorization
    fwd, rev = res["outcome"][:half], res["outcome"][half:]
    unit_answered = (fwd == F.DONE) | ((fwd == F.EMPTY) & (rev != F.HOST))
    out.update(candidates=int(len(cands)), factorizations=int(len(facts)), exons=int(len(fex)), outcomes=outcomes(res),
               branching={"patterns": int(branching.sum()), "outcomes": outcomes(res, branching), "units": int(unit_branching.sum()),
                          "units_neither_strand_host": int((unit_branching & ~unit_host).sum()),
                          "units_answered_forward_first": int((unit_branching & unit_answered).sum())},
               host_stage_1_details=np.bincount(res["detail"][(res["outcome"] == F.HOST) & (res["stage"] == 1)], minlength=3).tolist(),
               units_with_a_host_strand=int(unit_host.sum()), largest_list=int(res["n_listed"].max()),
               most_factorizations=int(res["n_facts"].max()),
               whole_call_ms=spread(ms[0]), clean_kernel_ms=spread(ms[1]), flist_select_kernel_ms=spread(ms[2]),
               gaps_kernel_ms=spread(ms[3]), chain_kernel_ms=spread(ms[4]), run_and_fetch_wall_ms=spread(wall),
               index_form_device_ms=spread(ix_dev), index_form_call_wall_ms=spread(ix_wall),
               host_ef_chain_factorizations_one_core_ms=round(host_ms, 2),
               host_note="through ctypes, one call per record, the oracle as the DP backend; its per-call cost is part of the figure")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
