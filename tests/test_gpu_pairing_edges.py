"""GPU: the pairing kernels (pgpu_pairing_plan.hip) on the edge cases of tests/pairing_edge_lib.py -- small
min_factor_len (the bisection without the 8-mer table below 8, the table's run taken whole at 8), matches laid against
the 16- and 32-base words of the packed sequences and against the ends of the genome and of the pattern blob, flagged
bytes, byte order, thresholds on the double's truncation, crowded position lists, odd batches.  Triples and `first`
offsets are compared exactly: with the committed fixture (tests/golden/pairing_edges.json.gz, answered by the
reference), and on fresh seeds with the oracle computed on the spot."""
import os

import numpy as np
import pytest

import pairing_edge_lib as E

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RELOADED = ("small_L", "windows", "flagged")


@pytest.fixture(scope="module")
def fixture():
    return E.load_fixture(os.path.join(GOLD, "pairing_edges.json.gz"))


def check(plan, want, label):
    """the plan's triples and first offsets against `want` = the pairings of every pattern, as nested lists"""
    tri, first = plan.fetch()
    exp_first = np.cumsum([0] + [len(w) for w in want])
    if first.tolist() != exp_first.tolist() or tri.tolist() != [r for w in want for r in w]:
        for k, w in enumerate(want):
            a, b = int(first[k]), int(first[k + 1])
            got = tri[a:b].tolist() if a <= b <= len(tri) else None
            if got != w or a != exp_first[k]:
                raise AssertionError("%s: pattern %d of %d: first %d..%d (expected %d..%d), got %r, expected %r"
                                     % (label, k, len(want), a, b, exp_first[k], exp_first[k + 1], got and got[:6], w[:6]))
        raise AssertionError("%s: first offsets differ: %r" % (label, first.tolist()[-3:]))


def run_case(ctx, idx, case, stored, resident=False):
    import pintron_amd.capi as capi
    name, _, ests, params = case
    for (L, rate), want in zip(params, stored):                              # one plan per (genome, L, rate)
        plan = capi.PairingPlan(ctx, idx, ests, resident=resident)
        try:
            plan.run(L, rate)
            check(plan, want, "%s L=%d rate=%s" % (name, L, rate))
        finally:
            plan.close()


@pytest.mark.parametrize("group", E.GROUPS)
def test_fixture(gpu_ctx, fixture, group):
    import pintron_amd.capi as capi
    for case, stored, _ in fixture[group]:
        idx = capi.Index(gpu_ctx, case[1])
        try:
            run_case(gpu_ctx, idx, case, stored)
        finally:
            idx.close()


@pytest.mark.parametrize("group", RELOADED)
def test_fixture_on_a_reloaded_index_and_resident_plans(gpu_ctx, fixture, group, tmp_path):
    """The index saved and read back (klo and khi come from the file), under an ordinary plan and under a resident one,
    whose patterns lie in one allocation with the offsets and the packed words behind them and whose buffers another
    resident plan, of another size, has written in between."""
    import pintron_amd.capi as capi
    path = str(tmp_path / "edge.idx")
    for case, stored, _ in fixture[group]:
        name, gen, ests, params = case
        built = capi.Index(gpu_ctx, gen)
        built.save(path)
        built.close()
        idx = capi.Index(gpu_ctx, gen, load_from=path)
        try:
            run_case(gpu_ctx, idx, case, stored)
            order = list(range(len(ests)))[::-1] + [0]                       # the second plan: other patterns, another size
            a = capi.PairingPlan(gpu_ctx, idx, ests, resident=True)
            b = capi.PairingPlan(gpu_ctx, idx, [ests[k] for k in order], resident=True)
            try:
                for (L, rate), want in zip(params, stored):
                    a.run(L, rate)
                    b.run(L, rate)
                    check(b, [want[k] for k in order], "%s (second resident plan) L=%d rate=%s" % (name, L, rate))
                    a.run(L, rate)
                    check(a, want, "%s (resident) L=%d rate=%s" % (name, L, rate))
            finally:
                a.close()
                b.close()
        finally:
            idx.close()


def test_one_plan_rerun_at_other_lengths(gpu_ctx, fixture):
    """The 129 patterns of `batch` in ONE plan, run at min_factor_len 7, 33, 8, 15, 2, 15: the lo, hi and thr of the run
    before are still in the buffers, and the candidate and output buffers grow (L = 2) and are used again smaller.  Each
    answer is a fresh plan's, and the oracle's."""
    import pintron_amd.capi as capi
    (case,) = [c for c, _, _ in fixture["batch"] if len(c[2]) == 129]
    _, gen, ests, _ = case
    idx = capi.Index(gpu_ctx, gen)
    plan = capi.PairingPlan(gpu_ctx, idx, ests)
    try:
        for step, L in enumerate(E.BATCH_LS):
            plan.run(L, 0.2)
            tri, first = plan.fetch()
            fresh = capi.PairingPlan(gpu_ctx, idx, ests)
            try:
                fresh.run(L, 0.2)
                ftri, ffirst = fresh.fetch()
            finally:
                fresh.close()
            assert np.array_equal(first, ffirst) and np.array_equal(tri, ftri), (step, L)
            (want,) = E.oracle_answers(gen, ests, [(L, 0.2)])
            check(plan, [w.tolist() for w in want], "step %d, L=%d" % (step, L))
            assert len(tri) > 0
    finally:
        plan.close()
        idx.close()


@pytest.mark.parametrize("group", E.GROUPS)
def test_fresh_cases_vs_oracle(gpu_ctx, group):
    """300 cases of the group from seeds the fixture does not hold, against the oracle computed here"""
    import pintron_amd.capi as capi
    n = 0
    for case in E.fresh_cases(group, 300):
        stored = [[w.tolist() for w in per_est] for per_est in E.oracle_answers(case[1], case[2], case[3])]
        idx = capi.Index(gpu_ctx, case[1])
        try:
            run_case(gpu_ctx, idx, case, stored)
        finally:
            idx.close()
        n += 1
    assert n == 300


def test_meg_stage_runs_behind_small_min_factor_len(gpu_ctx, fixture):
    """run_meg behind the pairings of min_factor_len 7 and 8, default parameters otherwise: PGPU_OK, and every record
    either available or flagged PGPU_MEG_UNAVAILABLE (a bare header).  What an available record holds is meg_lib's to say."""
    import struct
    import pintron_amd.capi as capi
    n = 0
    for case, _, _ in fixture["small_L"]:
        _, gen, ests, params = case
        if params[0][0] not in (7, 8):
            continue
        idx = capi.Index(gpu_ctx, gen)
        plan = capi.PairingPlan(gpu_ctx, idx, ests)
        try:
            for L, rate in params:
                plan.run(L, rate)
                plan.run_meg(min_factor_len=L)                                # raises unless PGPU_OK
                recs = plan.fetch_meg()
                assert len(recs) == len(ests)
                for k, rec in enumerate(recs):
                    nv, ne, flags, zero = struct.unpack_from("<4I", rec, 0)
                    assert flags & ~3 == 0 and zero == 0, (L, k, flags)
                    if flags & 2:
                        assert len(rec) == 16, (L, k, len(rec))
                    else:
                        assert nv <= 64 and len(rec) >= 16 + 12 * nv + 2 * (nv + 1) + ne + 8, (L, k, nv, ne, len(rec))
                        assert len(capi.parse_meg_record(rec)["vertices"]) == nv
                    n += 1
        finally:
            plan.close()
            idx.close()
    assert n >= 40
