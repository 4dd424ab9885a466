"""GPU: the order of calls on one pairing plan.  A plan holds the results of its stages as a ladder -- nothing <
pairings < records < candidates < factorizations -- and the rule is stated once (pintron_amd/csrc/pgpu_pairing_plan.hip):
a run of stage k first lowers the plan to k - 1, then asks for stage k - 1 (with the min_factor_len it was made with,
where the stage has one), and raises the plan to k when it succeeds; a fetch of stage k asks for stage k.  The refusal
tests of test_gpu_meg.py, test_gpu_cand.py and test_gpu_fact.py walk one path each; here one seeded walk of 3 000 calls
takes every call at every rung, against a model of the rule.

None of the eleven calls lowers a plan to `nothing` (run is never refused here), so that rung exists on a fresh plan only:
the walk replaces its plan by a fresh one over the same patterns at seeded moments, about once in 40 calls.

Before the ladder (four booleans, no check in the two older fetches) this walk met PGPU_OK in 159 of its calls where
the model refuses -- fetch at `nothing`, fetch_meg at `pairings` -- and agreed everywhere else."""
import ctypes as C
import random

import numpy as np
import pytest

import fact_lib as F
import meg_lib as M

pytestmark = pytest.mark.gpu

N_SEQS = 14         # the fewest leading sequences of meg_lib.rerun_input() with all four totals above 0, at L = 15 and at L = 16
N_OPS, SEED, RENEW = 3000, 19, 40
NOTHING, PAIRINGS, RECORDS, CANDIDATES, FACTORIZATIONS = range(5)
OPS = [("run", 15), ("run", 16), ("run_meg", 15), ("run_meg", 16), ("run_candidates", 15), ("run_candidates", 16),
       ("run_factorizations", None), ("fetch", None), ("fetch_meg", None), ("fetch_candidates", None),
       ("fetch_factorizations", None)]
STAGE_OF = dict(run=PAIRINGS, run_meg=RECORDS, run_candidates=CANDIDATES, run_factorizations=FACTORIZATIONS,
                fetch=PAIRINGS, fetch_meg=RECORDS, fetch_candidates=CANDIDATES, fetch_factorizations=FACTORIZATIONS)
PHRASE = dict(run_meg="run_meg needs the pairings of pgpu_pairing_plan_run with the same min_factor_len",
              run_candidates="run_candidates needs the records of pgpu_pairing_plan_run_meg with the same min_factor_len",
              run_factorizations="run_factorizations needs the candidates of pgpu_pairing_plan_run_candidates",
              fetch="fetch needs pgpu_pairing_plan_run first", fetch_meg="fetch_meg needs pgpu_pairing_plan_run_meg first",
              fetch_candidates="fetch_candidates needs pgpu_pairing_plan_run_candidates first",
              fetch_factorizations="fetch_factorizations needs pgpu_pairing_plan_run_factorizations first")


class Model:
    """The ladder: the rung, the min_factor_len of the pairings and of the records, and which totals are above 0."""

    def __init__(self):
        self.rung, self.L = NOTHING, {PAIRINGS: None, RECORDS: None}
        self.total = {k: False for k in range(PAIRINGS, FACTORIZATIONS + 1)}

    def apply(self, name, L):
        """True when the call must succeed, False when it must be PGPU_EINVAL with PHRASE[name]."""
        k = STAGE_OF[name]
        if name.startswith("fetch"):
            return self.rung >= k
        self.rung = min(self.rung, k - 1)                                  # lowered first, refused or not
        ok = self.rung == k - 1 and (k not in (RECORDS, CANDIDATES) or self.L[k - 1] == L)
        if ok:
            self.rung = k
            if k in self.L:
                self.L[k] = L
        self.total[k] = ok                                                 # a run resets its own total, and only that
        return ok


class Device:
    """One ordinary plan and the buffers its fetches fill, through the C entries (no exception in the way of a code)."""

    def __init__(self, ctx, idx, seqs):
        import pintron_amd.capi as capi
        self.capi, self.ctx, self.L_, self.n_pat = capi, ctx, ctx.L, len(seqs)
        self.plan = capi.PairingPlan(ctx, idx, seqs)
        self.first = np.zeros(self.n_pat + 1, dtype=np.uint64)
        self.got = {}

    def totals(self):
        h = self.plan.h
        return {PAIRINGS: self.L_.pgpu_pairing_plan_count(h), RECORDS: self.L_.pgpu_pairing_plan_meg_bytes(h),
                CANDIDATES: self.L_.pgpu_pairing_plan_candidate_exons(h), FACTORIZATIONS: self.L_.pgpu_pairing_plan_factorization_exons(h)}

    def message(self):
        return self.L_.pgpu_last_error(self.ctx.h).decode()

    def call(self, name, L):
        capi, L_, c, h, n = self.capi, self.L_, self.ctx.h, self.plan.h, self.totals()
        first = self.first.ctypes.data_as(C.POINTER(C.c_uint64))
        if name == "run":
            return L_.pgpu_pairing_plan_run(c, h, C.byref(capi.PairingParams(L, 0, 0.2)))
        if name == "run_meg":
            return L_.pgpu_pairing_plan_run_meg(c, h, C.byref(capi.MegParams(L, 40, 0, 80, 0.6, 0.6, 0.4, 1, 1)))
        if name == "run_candidates":
            return L_.pgpu_pairing_plan_run_candidates(c, h, C.byref(capi.CandParams(L, 40)))
        if name == "run_factorizations":
            return L_.pgpu_pairing_plan_run_factorizations(c, h, C.byref(capi.FactParams(*F.DEFAULTS)))
        if name == "fetch":
            out = np.zeros((n[PAIRINGS] + 1, 3), dtype=np.int32)
            rc = L_.pgpu_pairing_plan_fetch(c, h, out.ctypes.data_as(C.POINTER(capi.Pairing)), n[PAIRINGS] + 1, first)
            self.got[name] = (out[:n[PAIRINGS]].tobytes(), self.first.tobytes())
        elif name == "fetch_meg":
            out = np.zeros(n[RECORDS] + 1, dtype=np.uint8)
            rc = L_.pgpu_pairing_plan_fetch_meg(c, h, out.ctypes.data_as(C.c_void_p), n[RECORDS] + 1, first)
            self.got[name] = (out[:n[RECORDS]].tobytes(), self.first.tobytes())
        elif name == "fetch_candidates":
            res = np.zeros(self.n_pat, dtype=np.dtype(capi.CAND_RESULT_DTYPE))
            ex = np.zeros(n[CANDIDATES] + 1, dtype=np.dtype(capi.FACTOR_DTYPE))
            rc = L_.pgpu_pairing_plan_fetch_candidates(c, h, res.ctypes.data_as(C.POINTER(capi.CandResult)),
                                                       ex.ctypes.data_as(C.POINTER(capi.Factor)), n[CANDIDATES] + 1)
            self.got[name] = (res.tobytes(), ex[:n[CANDIDATES]].tobytes())
        else:
            res = np.zeros(self.n_pat, dtype=np.dtype(capi.FACT_RESULT_DTYPE))
            ex = np.zeros(n[FACTORIZATIONS] + 1, dtype=np.dtype(capi.FACTOR_DTYPE))
            st = np.zeros(n[FACTORIZATIONS] + 1, dtype=np.uint8)
            rc = L_.pgpu_pairing_plan_fetch_factorizations(c, h, res.ctypes.data_as(C.POINTER(capi.FactResult)),
                                                           ex.ctypes.data_as(C.POINTER(capi.Factor)),
                                                           st.ctypes.data_as(C.POINTER(C.c_uint8)), n[FACTORIZATIONS] + 1)
            self.got[name] = (res.tobytes(), ex[:n[FACTORIZATIONS]].tobytes(), st[:n[FACTORIZATIONS]].tobytes())
        return rc

    def full_answer(self):
        """run, run_meg, run_candidates, run_factorizations at L = 15, and what the four fetches give"""
        for name, L in (("run", 15), ("run_meg", 15), ("run_candidates", 15), ("run_factorizations", None),
                        ("fetch", None), ("fetch_meg", None), ("fetch_candidates", None), ("fetch_factorizations", None)):
            assert self.call(name, L) == self.capi.PGPU_OK, (name, self.message())
        return dict(self.got)


def test_every_call_at_every_rung(gpu_ctx):
    import pintron_amd.capi as capi
    gfa, efa = M.rerun_input()
    exp, genomic = M.first_attempt_megs(gfa, efa)
    seqs = [e["seq"] for e in exp][:N_SEQS]
    idx = capi.Index(gpu_ctx, genomic)
    rng = random.Random(SEED)
    dev, model, seen, wrong = Device(gpu_ctx, idx, seqs), Model(), set(), []
    try:
        for step in range(N_OPS):
            if rng.randrange(RENEW) == 0:
                dev.plan.close()
                dev, model = Device(gpu_ctx, idx, seqs), Model()
            name, L = rng.choice(OPS)
            before = model.rung
            seen.add((before, name, L))
            ok = model.apply(name, L)
            rc = dev.call(name, L)
            where = (step, before, name, L)
            if rc != (capi.PGPU_OK if ok else capi.PGPU_EINVAL) or (not ok and PHRASE[name] not in dev.message()):
                wrong.append(where + (rc, dev.message() if rc else ""))
            assert {k: v > 0 for k, v in dev.totals().items()} == model.total, where
        print("calls the model answers otherwise: %d" % len(wrong))
        for w in wrong[:20]:
            print("  step %d, rung %d, %s(%s): rc %d %r" % w)
        assert not wrong, wrong[:5]
        assert seen == {(rung, name, L) for rung in range(5) for name, L in OPS}
        last = dev.full_answer()
        fresh = Device(gpu_ctx, idx, seqs)
        try:
            want = fresh.full_answer()
        finally:
            fresh.plan.close()
        assert all(len(want[k][0]) > 0 for k in want) and last == want
    finally:
        dev.plan.close()
        idx.close()
