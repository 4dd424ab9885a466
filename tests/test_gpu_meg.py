"""GPU: the device MEG stage (pgpu_pairing_plan_run_meg) at its caps, under every parameter, on reruns.
The expectation is the host MEG code over the pairing oracle (tests/hostcheck/meg_check); the inputs, the parameter
sets and the rule that says when a record must, or must not, be PGPU_MEG_UNAVAILABLE are in tests/meg_lib.py, and
tests/test_meg_cases_cpu.py proves without a GPU that every input reaches the edge it is aimed at."""
import ctypes as C

import numpy as np
import pytest

import meg_lib as M

pytestmark = pytest.mark.gpu


def _seqs(exp):
    return [e["seq"] for e in exp]


@pytest.mark.parametrize("source", ["c2", "repeats"])
def test_parameter_sweep(gpu_ctx, source):
    """Every field of pgpu_meg_params off its default, the pairings run at the set's min_factor_len: flags by the
    rule, available records exact.  Grey records (within the caps, DFS stack bound not shown) are counted."""
    import pintron_amd.capi as capi
    gfa, efa, exons = M.sweep_sources()[source]
    base, genomic = M.first_attempt_megs(gfa, efa)
    idx = capi.Index(gpu_ctx, genomic)
    try:
        for name, prm in [("defaults", M.DEFAULTS)] + M.sweep_sets(exons):
            exp, _ = M.first_attempt_megs(gfa, efa, prm)
            assert _seqs(exp) == _seqs(base)
            plan = capi.PairingPlan(gpu_ctx, idx, _seqs(exp))
            try:
                plan.run(prm["min_factor_len"], 0.2)
                plan.run_meg(**prm)
                recs = [M.parse_record(r) for r in plan.fetch_meg()]
            finally:
                plan.close()
            grey = M.check_records(exp, recs, prm, (source, name))
            n_un = sum(r["flags"] & 2 != 0 for r in recs)
            print("%s %s: %d records, %d unavailable, %d grey" % (source, name, len(recs), n_un, grey))
            assert grey * 20 <= len(exp) and n_un * 20 <= len(exp), (source, name, grey, n_un)
    finally:
        idx.close()


@pytest.mark.parametrize("name", [n for n, _ in M.CRAFTED_SETS])
def test_caps(gpu_ctx, name):
    """61 / 62 / 63 pairings, lists of 32 / 33, the compaction that carries the vertex count over 64 (and the same
    input with the compaction off), tp >= 50: the over-cap patterns are flagged, nothing else is, and their
    neighbours in the plan (the scratch blocks lie side by side) are exact.  No record is grey."""
    prm = dict(M.CRAFTED_SETS)[name]
    gfa, efa, labels = M.crafted()
    exp, genomic = M.first_attempt_megs(gfa, efa, prm)
    recs = M.device_records(gpu_ctx, genomic, _seqs(exp), prm)
    assert M.check_records(exp, recs, prm, name) == 0
    flagged = [l for l, r in zip(labels, recs) if r["flags"] & 2]
    print(name, "unavailable:", flagged)
    assert flagged and "ordinary" not in flagged


@pytest.mark.parametrize("n_pat", [1, 64, 65])
def test_degenerate_patterns(gpu_ctx, n_pat):
    """Patterns of L - 1, L and L + 1 bases, without a pairing, of Ns only, among ordinary ones; plans of one
    pattern, of one full block of the kernel, and of one block plus one."""
    gfa, efa = M.degenerate(n_pat)
    exp, genomic = M.first_attempt_megs(gfa, efa)
    assert len(exp) == n_pat
    for resident in (False, True):
        recs = M.device_records(gpu_ctx, genomic, _seqs(exp), M.DEFAULTS, resident=resident)
        assert M.check_records(exp, recs, M.DEFAULTS, (n_pat, resident)) == 0
        assert not any(r["flags"] & 2 for r in recs)


def test_empty_plan(gpu_ctx):
    import pintron_amd.capi as capi
    idx = capi.Index(gpu_ctx, b"ACGTTGCATGCATGCCGTA" * 20)
    for resident in (False, True):
        plan = capi.PairingPlan(gpu_ctx, idx, [], resident=resident)
        try:
            prm = capi.MegParams(15, 40, 0, 80, 0.6, 0.6, 0.4, 1, 1)
            assert gpu_ctx.L.pgpu_pairing_plan_run_meg(gpu_ctx.h, plan.h, C.byref(prm)) == capi.PGPU_OK
            assert gpu_ctx.L.pgpu_pairing_plan_meg_bytes(plan.h) == 0
            first = np.full(1, 77, dtype=np.uint64)
            assert gpu_ctx.L.pgpu_pairing_plan_fetch_meg(gpu_ctx.h, plan.h, None, 0, first.ctypes.data_as(C.POINTER(C.c_uint64))) == capi.PGPU_OK
            assert first[0] == 0
            assert plan.fetch_meg() == []
        finally:
            plan.close()
    idx.close()


@pytest.fixture(scope="module")
def rerun_case():
    """An input whose records are several times larger without the simplifications, and its expectations at
    L = 15, L = 16 and with both simplifications off."""
    gfa, efa = M.rerun_input()
    sets = dict(d15=M.DEFAULTS, d16=M.params(min_factor_len=16), neither=M.NEITHER)
    exp = {k: M.first_attempt_megs(gfa, efa, p)[0] for k, p in sets.items()}
    genomic = M.first_attempt_megs(gfa, efa)[1]
    return genomic, _seqs(exp["d15"]), sets, exp


def _run_and_check(plan, sets, exp, key, run_pairings=True):
    if run_pairings:
        plan.run(sets[key]["min_factor_len"], 0.2)
    n = plan.run_meg(**sets[key])
    raw = plan.fetch_meg()
    assert sum(len(r) for r in raw) == n
    assert M.check_records(exp[key], [M.parse_record(r) for r in raw], sets[key], key) == 0
    return raw, n


@pytest.mark.parametrize("resident", [False, True])
def test_reruns_on_one_plan(gpu_ctx, rerun_case, resident):
    import pintron_amd.capi as capi
    genomic, seqs, sets, exp = rerun_case
    idx = capi.Index(gpu_ctx, genomic)
    fresh = {}
    for key in sets:                                               # a fresh ordinary plan each: what a rerun must equal
        p = capi.PairingPlan(gpu_ctx, idx, seqs)
        fresh[key] = _run_and_check(p, sets, exp, key)[0]
        p.close()
    plan = capi.PairingPlan(gpu_ctx, idx, seqs, resident=resident)
    try:
        # other parameters for the pairings and back
        for key in ("d15", "d16", "d15"):
            assert _run_and_check(plan, sets, exp, key)[0] == fresh[key], key
        # the MEG stage three times on the same pairings; the middle run's records are larger than the buffer of the first
        sizes = []
        for key in ("d15", "neither", "d15"):
            raw, n = _run_and_check(plan, sets, exp, key, run_pairings=False)
            assert raw == fresh[key], key
            sizes.append(n)
        assert sizes[1] > sizes[0] + sizes[0] // 8 + 4096 and sizes[2] == sizes[0]       # past the slack run_meg allocates
        # a buffer one byte short, then the right one
        n = gpu_ctx.L.pgpu_pairing_plan_meg_bytes(plan.h)
        out = np.zeros(n, dtype=np.uint8)
        first = np.zeros(len(seqs) + 1, dtype=np.uint64)
        rc = gpu_ctx.L.pgpu_pairing_plan_fetch_meg(gpu_ctx.h, plan.h, out.ctypes.data_as(C.c_void_p), n - 1,
                                                   first.ctypes.data_as(C.POINTER(C.c_uint64)))
        assert rc == capi.PGPU_ENOSPC and not out.any()
        assert plan.fetch_meg() == fresh["d15"]
    finally:
        plan.close()
        idx.close()


def test_refusals(gpu_ctx, rerun_case):
    """run_meg without pairings, with another min_factor_len than the pairings', with min_factor_len 0: PGPU_EINVAL,
    and the same context and plan answer correctly afterwards."""
    import pintron_amd.capi as capi
    genomic, seqs, sets, exp = rerun_case
    message = "run_meg needs the pairings of pgpu_pairing_plan_run with the same min_factor_len"
    idx = capi.Index(gpu_ctx, genomic)
    plan = capi.PairingPlan(gpu_ctx, idx, seqs)
    try:
        with pytest.raises(capi.PgpuError) as e:                   # before any run
            plan.run_meg()
        assert e.value.code == capi.PGPU_EINVAL and message in str(e.value)
        want = _run_and_check(plan, sets, exp, "d15")[0]
        with pytest.raises(capi.PgpuError) as e:                   # another L than the last run's
            plan.run_meg(**sets["d16"])
        assert e.value.code == capi.PGPU_EINVAL and message in str(e.value)
        assert _run_and_check(plan, sets, exp, "d15", run_pairings=False)[0] == want
        prm = capi.MegParams(0, 40, 0, 80, 0.6, 0.6, 0.4, 1, 1)
        assert gpu_ctx.L.pgpu_pairing_plan_run_meg(gpu_ctx.h, plan.h, C.byref(prm)) == capi.PGPU_EINVAL
        assert _run_and_check(plan, sets, exp, "d15", run_pairings=False)[0] == want
        assert _run_and_check(plan, sets, exp, "d16")[0] != want
        with pytest.raises(capi.PgpuError) as e:                   # the pairings are those of L = 16 now
            plan.run_meg(**sets["d15"])
        assert e.value.code == capi.PGPU_EINVAL and message in str(e.value)
        assert _run_and_check(plan, sets, exp, "d15")[0] == want
    finally:
        plan.close()
        idx.close()
